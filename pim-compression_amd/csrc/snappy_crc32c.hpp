// snappy_crc32c.hpp -- CRC-32C (Castagnoli, reflected 0x82F63B78) by one wavefront, and the batch kernel of
// snappy_hip_crc32c_batch (include/snappy_hip.h).  gfx950 has neither a carry-less multiply nor a CRC instruction.
//
// crc32c_wave: the n bytes are cut into 64 contiguous pieces.  Lanes 1..63 take S = 4 * (n / 256) bytes each, the LAST 63 S bytes
// of the buffer; lane 0 takes what is in front of them, n - 63 S bytes (S .. S + 255): the ragged piece is the FIRST one, so
// every piece behind it has one length and the join needs no shift by a variable distance.  A lane walks its piece through a
// table in LDS (crc_walk), lane 0 from the caller's seed, the others from 0.  The 64 partial states are joined by the
// linearity of the CRC: a state followed by k zero bytes is its product with x^(8k) mod P in GF(2)[x] (gf_mul), so a
// Hillis-Steele scan of six rounds -- lane l takes lane l - d's state times x^(8 S d), d = 1, 2, .. 32 -- leaves the CRC of the
// whole buffer in lane 63.  x^(8 S) is the product of the x^(2^k) (x2n) over the bits of 8 S; each round squares it.
//
// kTables: 1 = a 256-entry byte table (1 KiB of LDS, one dependent look-up per byte), 4 = slicing-by-4 (4 KiB, four
// independent look-ups per 4 bytes).  crc_table_init fills either; DESIGN.md 3.12 has the choice and its numbers.
#pragma once
#include "snappy_device_common.hpp"

namespace snappy_hip {

constexpr uint32_t kCrcPoly = 0x82F63B78u;
constexpr uint32_t kCrcMaskDelta = 0xa282ead8u;

// the masked form a CRC is stored in by the framing format
__host__ __device__ inline uint32_t crc_mask(uint32_t c) { return ((c >> 15) | (c << 17)) + kCrcMaskDelta; }

// a * b mod P; bit 31 is the coefficient of x^0 (the reflected form the CRC state is kept in)
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}

// x^(2^k) mod P, k = 0..31 (tests/test_sz_model.py recomputes them)
__device__ __forceinline__ uint32_t x2n(uint32_t k)
{
    switch (k & 31u) {
    case 0: return 0x40000000u;
    case 1: return 0x20000000u;
    case 2: return 0x08000000u;
    case 3: return 0x00800000u;
    case 4: return 0x00008000u;
    case 5: return 0x82f63b78u;
    case 6: return 0x6ea2d55cu;
    case 7: return 0x18b8ea18u;
    case 8: return 0x510ac59au;
    case 9: return 0xb82be955u;
    case 10: return 0xb8fdb1e7u;
    case 11: return 0x88e56f72u;
    case 12: return 0x74c360a4u;
    case 13: return 0xe4172b16u;
    case 14: return 0x0d65762au;
    case 15: return 0x35d73a62u;
    case 16: return 0x28461564u;
    case 17: return 0xbf455269u;
    case 18: return 0xe2ea32dcu;
    case 19: return 0xfe7740e6u;
    case 20: return 0xf946610bu;
    case 21: return 0x3c204f8fu;
    case 22: return 0x538586e3u;
    case 23: return 0x59726915u;
    case 24: return 0x734d5309u;
    case 25: return 0xbc1ac763u;
    case 26: return 0x7d0722ccu;
    case 27: return 0xd289cabeu;
    case 28: return 0xe94ca9bcu;
    case 29: return 0x05b74f3fu;
    case 30: return 0xa51e1f42u;
    default: return 0x40000000u;         // x^(2^31): the order of x divides 2^32 - 1
    }
}

// x^(32 words) mod P: the operator of `words` zero words behind a state; words < 2^27
__device__ __forceinline__ uint32_t x_pow_words(uint32_t words)
{
    uint32_t r = 0x80000000u;            // x^0
    for (uint32_t k = 5; words; ++k, words >>= 1)
        if (words & 1u) r = gf_mul(r, x2n(k));
    return r;
}

// LDS words the tables take
template <int kTables>
constexpr uint32_t crc_table_words() { return 256u * kTables; }

// Fills the tables (every lane of a 64-lane wavefront calls it): T0[b] = the state after byte b from state 0, Tj[b] =
// T0[b] followed by j zero bytes.  The caller puts a barrier between this and the first crc32c_wave.
template <int kTables>
__device__ __forceinline__ void crc_table_init(uint32_t* table, uint32_t lane)
{
    for (uint32_t b = lane; b < 256u; b += kWave) {
        uint32_t c = b;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
        table[b] = c;
        for (int j = 1; j < kTables; ++j) {
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
            table[256 * j + b] = c;
        }
    }
}

template <int kTables>
__device__ __forceinline__ uint32_t crc_word(uint32_t c, uint32_t w, const uint32_t* table)
{
    c ^= w;
    if constexpr (kTables == 4) {
        return table[768u + (c & 0xffu)] ^ table[512u + ((c >> 8) & 0xffu)] ^ table[256u + ((c >> 16) & 0xffu)] ^ table[c >> 24];
    } else {
        c = (c >> 8) ^ table[c & 0xffu];
        c = (c >> 8) ^ table[c & 0xffu];
        c = (c >> 8) ^ table[c & 0xffu];
        return (c >> 8) ^ table[c & 0xffu];
    }
}

// one lane's piece: len bytes at p (any alignment), not one byte read beyond them
template <int kTables>
__device__ __forceinline__ uint32_t crc_walk(uint32_t c, const uint8_t* p, uint32_t len, const uint32_t* table)
{
    uint32_t i = 0;
    for (; i + 16u <= len; i += 16u) {
        const uint4 v = ld128(p + i);
        c = crc_word<kTables>(c, v.x, table);
        c = crc_word<kTables>(c, v.y, table);
        c = crc_word<kTables>(c, v.z, table);
        c = crc_word<kTables>(c, v.w, table);
    }
    for (; i + 4u <= len; i += 4u) c = crc_word<kTables>(c, ld32(p + i), table);
    for (; i < len; ++i) c = (c >> 8) ^ table[(c ^ p[i]) & 0xffu];
    return c;
}

// The CRC state after the n bytes at p, from `seed`, in every lane.  p, n, seed wave-uniform; every lane of the wavefront
// calls it; n < 2^31.  The CRC-32C of a buffer is ~crc32c_wave(0xffffffff, ...); a long buffer may be fed in pieces, each
// from the state the one before left.
template <int kTables>
__device__ __forceinline__ uint32_t crc32c_wave(uint32_t seed, const uint8_t* p, uint32_t n, uint32_t lane, const uint32_t* table)
{
    const uint32_t words = n >> 8;                   // S / 4
    const uint32_t S = words << 2;
    const uint32_t head = n - 63u * S;
    uint32_t v;
    if (lane == 0) v = crc_walk<kTables>(seed, p, head, table);
    else v = crc_walk<kTables>(0u, p + head + (lane - 1u) * S, S, table);
    if (words == 0) return uni(v);                   // (lane 0 had it all)
    uint32_t op = x_pow_words(words);                // x^(8 S d), d = 1
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const uint32_t from = (uint32_t)__shfl_up((int)v, (int)d);
        const uint32_t joined = gf_mul(op, from) ^ v;
        if (lane >= d) v = joined;
        op = gf_mul(op, op);
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

struct CrcItem {                // must match snappy_hip_crc_item (include/snappy_hip.h)
    const uint8_t* src;
    uint64_t src_len;
};

// The table form the product runs: the byte table.  Measured: the CRC alone runs at the same rate in both forms,
// and the decode kernel with slicing-by-4's 4 KiB beside K2's stage no longer holds eight wavefronts per SIMD in a CU's LDS.
#ifndef SNAPPY_CRC_TABLES
#define SNAPPY_CRC_TABLES 1
#endif
constexpr int kCrcTables = SNAPPY_CRC_TABLES;

// the longest piece crc32c_wave is fed at once
constexpr uint64_t kCrcPiece = 1ull << 30;

// the CRC-32C of n bytes of any length (wave-uniform arguments, the result in every lane)
template <int kTables>
__device__ __forceinline__ uint32_t crc32c_wave_long(const uint8_t* p, uint64_t n, uint32_t lane, const uint32_t* table)
{
    uint32_t c = 0xffffffffu;
    do {
        const uint32_t piece = n < kCrcPiece ? (uint32_t)n : (uint32_t)kCrcPiece;
        c = crc32c_wave<kTables>(c, p, piece, lane, table);
        p += piece;
        n -= piece;
    } while (n);
    return ~c;
}

// Persistent wavefronts draw items: crc[i] = the (unmasked) CRC-32C of item i's src[0, src_len); 0 for an empty item.
template <int kTables>
__global__ __launch_bounds__(64) void crc32c_batch_kernel(const CrcItem* __restrict__ items, uint32_t count, uint32_t* __restrict__ crc,
                                                          uint32_t* next_item)
{
    __shared__ uint32_t table[crc_table_words<kTables>()];
    const uint32_t lane = threadIdx.x;
    crc_table_init<kTables>(table, lane);
    __syncthreads();
    for (;;) {
        const uint32_t i = draw_work(next_item, lane);
        if (i >= count) break;
        const uint8_t* src = load_global_ptr(&items[i].src);
        const uint64_t n = src ? uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len)) : 0;
        const uint32_t c = crc32c_wave_long<kTables>(src, n, lane, table);
        if (lane == 0) crc[i] = c;
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace snappy_hip
