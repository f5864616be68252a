// snappy_k2_wide.hpp -- ONE framed block decoded by a whole workgroup (snappy_hip_decompress_blocks_wide, include/snappy_hip.h;
// DESIGN.md 3.10).
//
// K2 (decompress_blocks_kernel) gives a block to one wavefront: a launch of a few blocks -- a small file -- is one block's
// element chain on one wavefront however many compute units sit idle.  A raw stream could be cut at fragment boundaries
// (snappy_raw_split.hpp); a block cannot, its copies reach anywhere in the block.  So the block's second half is different
// here: the elements are found by W wavefronts at once, and the back-references are resolved in parallel in LDS.
//
// One workgroup of W wavefronts (blockDim.x = 64 * W, W = 2, 4, 8 or 16) per block; persistent workgroups draw blocks from the
// launch's counter.  Everything between two draws happens inside the workgroup, separated by __syncthreads() only: no wait
// on another workgroup's or wavefront's flag.
//   A stage    the block's compressed bytes -> LDS, 16 bytes per thread; srcmap[i] = i.
//   B shares   the compressed bytes are cut into W shares on 64-byte boundaries.  Lane l of wavefront w walks the chain of
//              elements that would start at byte l of share w -- sizes only, read from LDS (wide_element_size, the rules of
//              predecode_window<false>) -- to the first position at or beyond the next share: table[w][l] = (landing, output
//              bytes), or "invalid".
//   C resolve  one thread follows the true chain from byte 0 across the shares, at most W steps: an entry inside a share's
//              first 64 bytes is a table lookup, an entry behind them (after a literal of more than 61 bytes) is walked from
//              there; a share the chain passes over gets no entry.  Each share gets (entry, output base, landing, output end).
//   D place    THE PROOF OF THE CHAIN.  Every wavefront walks its share again from its entry with K2's own window machinery
//              (predecode_window<false>, the doubled jump vector, k2_chain_walk and the fill-in, instantiated again, not
//              changed): every element is judged by the code that judges it in K2, with K2's tests -- an element predecode
//              rejects, output past out_len, a copy with offset 0 or reaching before the block's first byte.  A literal's
//              payload goes to out[], a copy sets srcmap[i] = i - offset for its bytes.  The share is accepted iff the walk
//              lands exactly on the landing and output end step C gave it, which are the next share's entry and base (csz and
//              out_len for the last one: step C tested that).
//   E resolve  srcmap[i] = srcmap[srcmap[i]] in rounds until nothing changes (at most 15 rounds for 32,768 bytes: a run of
//              32,767 bytes at offset 1 is the deepest chain), one barrier per round; then out[i] = out[srcmap[i]].
//   F store    out[0, out_len) -> the block's window in global memory, 16 bytes per thread on the aligned middle.
// When every share is accepted the shares' elements, in order, ARE the block's element stream, each passed K2's own tests, and
// their outputs tile [0, out_len): status OK and the bytes of the serial decode.  In every other case -- and for every block
// beyond the limits below -- wavefront 0 decodes the block with k2_decode_block<false> itself, in the same trip: every INVALID
// verdict is K2's own, and a mistake in steps B or C can cause a fallback, never a wrong byte.  The wide path writes nothing to
// global memory before step F.
//
// Limits of the wide path: block_size, and with it out_len, <= kWideMaxBlock (32,768: srcmap is u16; at a larger block size
// every block goes serial, a short last one too), the size word and the payload inside the stream,
// csz <= kWideMaxCsz (38,400 >= 32 + 32,768 + 32,768 / 6: every compressor-made block of at most 32 KiB).
// LDS, static, one workgroup per CU: compressed stage 38,528 (csz + the zeros window loads read behind it) + output 32,768 +
// srcmap 65,536 + share table 8,192 (K2's 1,536-byte stage for the fallback lies over it) + control words 384 = 145,408 of
// 163,840 bytes.
// Measured on one MI355X (tools/k2_wide_rate.py, profiles/k2_wide_rate.jsonl; data resident, 32 KiB blocks, ms, K2 / W = 4 / 8 / 16):
// terror2 (4 blocks) 0.402 / 0.441 / 0.273 / 0.238 -- the one case where the wide form wins (K2's run-to-run spread 4.8 %);
// dickens-size (312) 0.482 / 0.940 / 0.561 / 0.487; mozilla-size (1,564) 0.468 / 1.384 / 0.846 / 0.730; spamfile-size (2,571)
// 0.638 / 4.67 / 2.74 / 2.35; 1 GiB (32,768) 2.88 / 42.0 / 25.0 / 21.4.  The forms cross between 4 and 312 blocks: one
// workgroup per CU, so up to 256 blocks are one trip of ~0.24 ms and 312 are two.  Steps C and E do not shrink with W.
// d_result (u32, added to by one thread per block): [0] blocks the wide path decoded, [1] blocks sent to the serial decoder by
// the limits, [2] blocks the wide path did not prove.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_kernels.hpp"   // predecode_window, k2_chain_walk, k2_decode_block, lds_bytes_t

namespace snappy_hip {

constexpr uint32_t kWideMaxBlock = 32768;
constexpr uint32_t kWideMaxCsz = 38400;
constexpr uint32_t kWideMaxWaves = 16;
constexpr uint32_t kWideZone = 64;                   // table entries per share: one per lane
constexpr uint32_t kWideNone = 0xffffffffu;          // a share the true chain does not enter
constexpr uint64_t kWideInvalid = ~0ull;             // a table entry whose chain met an invalid element
constexpr uint32_t kWideRounds = 17;                 // 15 rounds of doubling, one that sees no change, one to spare

// the workgroup's LDS, byte offsets (every part a multiple of 16)
constexpr uint32_t kWideCompAt = 0;
constexpr uint32_t kWideCompBytes = kWideMaxCsz + 128;
constexpr uint32_t kWideOutAt = kWideCompAt + kWideCompBytes;
constexpr uint32_t kWideMapAt = kWideOutAt + kWideMaxBlock;
constexpr uint32_t kWideTableAt = kWideMapAt + 2 * kWideMaxBlock;
constexpr uint32_t kWideCtlAt = kWideTableAt + kWideMaxWaves * kWideZone * 8;
constexpr uint32_t kWideLdsBytes = kWideCtlAt + 384;
static_assert(kWideLdsBytes <= 160u * 1024u, "one workgroup per CU");
static_assert(kWideMaxWaves * kWideZone * 8 >= kK2StageBytes, "K2's stage lies over the share table");
// control words: [0, 16) entry, [16, 32) output base, [32, 48) landing, [48, 64) output end of each share; then
enum : uint32_t { kWideDrawn = 64, kWideBadC = 65, kWideBadD = 66, kWideChanged = 68 /* .. 68 + kWideRounds */ };

// LDS pointers that keep their address space (ds_* instead of flat_*); the CPU emulator sees plain pointers
#ifdef SNAPPY_EMU
#define SNAPPY_WIDE_LDS
typedef uint4 wide_v4_t;
#else
#define SNAPPY_WIDE_LDS __attribute__((address_space(3)))
typedef uint32_t wide_v4_t __attribute__((ext_vector_type(4)));      // (a plain vector: HIP's uint4 class has no LDS operator=)
#endif
typedef SNAPPY_WIDE_LDS uint8_t* wide_lds8_t;
typedef SNAPPY_WIDE_LDS uint16_t* wide_lds16_t;
typedef SNAPPY_WIDE_LDS uint32_t* wide_lds32_t;
typedef SNAPPY_WIDE_LDS uint64_t* wide_lds64_t;
typedef SNAPPY_WIDE_LDS wide_v4_t* wide_lds128_t;
typedef uint32_t __attribute__((aligned(1))) wide_u32_unaligned_t;
typedef wide_v4_t __attribute__((aligned(1))) wide_u128_unaligned_t;

__device__ __forceinline__ uint32_t wide_ld32u(wide_lds8_t p) { return *reinterpret_cast<SNAPPY_WIDE_LDS const wide_u32_unaligned_t*>(p); }
__device__ __forceinline__ void wide_st32u(wide_lds8_t p, uint32_t v) { *reinterpret_cast<SNAPPY_WIDE_LDS wide_u32_unaligned_t*>(p) = v; }

// Size of the element at comp[pos] as predecode_window<false> sizes it, by ONE lane for itself: consumed = its compressed
// bytes, olen = its output bytes.  False where predecode_window rejects: a literal of more than 65,536 bytes, or a header or a
// literal's payload running past csz.  Reads 5 bytes (the stage holds zeros behind csz).
__device__ __forceinline__ bool wide_element_size(wide_lds8_t comp, uint32_t pos, uint32_t csz, uint32_t& consumed, uint32_t& olen)
{
    const uint32_t lo = wide_ld32u(comp + pos);
    const uint32_t tag = lo & 0xffu;
    const uint32_t type = tag & 3u;
    const uint32_t v = tag >> 2;
    const uint32_t next4 = (lo >> 8) | ((uint32_t)comp[pos + 4] << 24);
    const bool lit = type == 0;
    const bool long_lit = lit && v >= 60u;
    const uint32_t raw = next4 & (0xffffffffu >> ((63u - v) * 8u & 31u));
    olen = (type == 1) ? (v & 7u) + 4u : v + 1u;
    olen = long_lit ? ((raw < 65536u) ? raw + 1u : 0u) : olen;
    const uint32_t hdr = long_lit ? v - 58u : (lit ? 1u : ((type == 3) ? 5u : type + 1u));
    consumed = hdr + (lit ? olen : 0u);
    return olen != 0 && pos + consumed <= csz;
}

// one lane's chain from `pos` to the first element start at or beyond `end` (<= csz): (landing | output bytes << 32) or kWideInvalid
__device__ __forceinline__ uint64_t wide_lane_walk(wide_lds8_t comp, uint32_t pos, uint32_t end, uint32_t csz)
{
    uint32_t out = 0;
    bool ok = true;
    while (pos < end) {
        uint32_t consumed, olen;
        if (!wide_element_size(comp, pos, csz, consumed, olen) || olen > kWideMaxBlock - out) {   // (more than any block here holds)
            ok = false;
            break;
        }
        pos += consumed;
        out += olen;
    }
    return ok ? ((uint64_t)pos | ((uint64_t)out << 32)) : kWideInvalid;
}

// Step D for one share: the elements of comp[entry, ...) walked by the whole wavefront, a 64-byte window at a time, up to the
// first element start at or beyond `limit` (entry < limit <= csz).  Literal payloads go to outb[], copies into srcmap[]; every
// write lies inside [0, out_len).  False when K2 would refuse an element here.  Wave-uniform arguments; every lane calls it.
// The window is k2_decode_block's, its bytes read from the stage (zeros behind csz: the verdict on an element never depends
// on bytes behind csz, an element that reaches them is rejected by its header).
__device__ __forceinline__ bool wide_share_walk(wide_lds8_t comp, uint32_t csz, uint32_t entry, uint32_t limit, uint32_t op0, uint32_t out_len,
                                                wide_lds8_t outb, wide_lds16_t srcmap, uint32_t lane, uint32_t& landing, uint32_t& op_end)
{
    uint32_t cp = entry, op = op0;
    bool ok = true;
    while (cp < limit) {                                             // one iteration per 64-byte window
        const uint32_t g = cp & ~63u;
        const uint64_t w0 = (uint64_t)wide_ld32u(comp + g + lane) | ((uint64_t)wide_ld32u(comp + g + lane + 4u) << 32);
        const uint32_t wend = (limit < g + 64) ? limit : g + 64;     // element starts at or beyond `limit` are the next share's
        const uint32_t wlim = wend - g;
        uint32_t e_type, e_hdr, e_len, e_consumed, offv;
        unsigned long long REJ;
        predecode_window<false>(w0, g + lane, csz, e_type, e_hdr, e_len, offv, e_consumed, REJ);
        const uint32_t advv = __builtin_amdgcn_inverse_ballot_w64(REJ) ? 64u : e_consumed;
        uint32_t s = cp - g;
        unsigned long long E = 0;
        {                                                            // the doubled jump vector and the fill-in, as K2 has them
            uint32_t jump[kK2WalkLevels + 1], tgt[kK2WalkLevels + 1];
            jump[0] = advv;
            tgt[0] = lane + advv;
#pragma unroll
            for (uint32_t k = 1; k <= kK2WalkLevels; ++k) {
                const uint32_t a_n = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(tgt[k - 1] << 2), (int)jump[k - 1]);
                jump[k] = jump[k - 1] + (tgt[k - 1] < wlim ? a_n : 0u);
                tgt[k] = lane + jump[k];
            }
            k2_chain_walk(jump[kK2WalkLevels], wlim, s, E);
#pragma unroll
            for (uint32_t k = kK2WalkLevels; k-- > 0;) {
                const bool pusher = __builtin_amdgcn_inverse_ballot_w64(E) && tgt[k] < wlim;
                const uint32_t got = (uint32_t)__builtin_amdgcn_ds_permute((int)(pusher ? tgt[k] << 2 : 0u), pusher ? 1 : 0);
                E |= __ballot(got != 0) & ~1ull;
            }
        }
        if (E & REJ) {                                               // an element predecode rejected
            ok = false;
            break;
        }
        const bool starts = __builtin_amdgcn_inverse_ballot_w64(E);
        const uint32_t mylen = starts ? e_len : 0u;
        const uint32_t incl = wave_inclusive_scan(mylen, lane);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t dstp = op + (incl - mylen);                   // where this lane's element starts in the block's output
        const unsigned long long COPY = E & __ballot(e_type != 0);
        if (total > out_len - op || (COPY & (__ballot(offv == 0) | __ballot(offv > dstp)))) {   // (op <= out_len throughout)
            ok = false;
            break;
        }
        // ---- literals: a payload byte of this window belongs to the last element that starts at or below its lane ----
        {
            const unsigned long long below = E & (~0ull >> (63u - lane));
            const bool any = below != 0;
            const uint32_t em = 63u - (uint32_t)__builtin_clzll(below | 1ull);
            const uint32_t packed = dstp | (e_hdr << 16) | (e_type << 20);                      // (dstp < 32,768 where an element has bytes)
            const uint32_t pk = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(em << 2), (int)packed);
            const uint32_t eat = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(em << 2), (int)e_consumed);
            const uint32_t pstart = em + ((pk >> 16) & 7u);
            if (any && ((pk >> 20) & 3u) == 0 && lane >= pstart && lane < em + eat) outb[(pk & 0xffffu) + lane - pstart] = (uint8_t)w0;
        }
        // ---- a last literal's run-on beyond the window: the wavefront copies it, a dword per lane and step ----
        if (s > 64u) {
            const uint32_t le = 63u - (uint32_t)__builtin_clzll(E);
            if ((uint32_t)__builtin_amdgcn_readlane((int)e_type, (int)le) == 0) {
                const uint32_t ps = le + (uint32_t)__builtin_amdgcn_readlane((int)e_hdr, (int)le);
                const uint32_t from = ps > 64u ? ps : 64u;           // a tag in the last lanes: payload from ps > 64
                const uint32_t n = s - from;
                wide_lds8_t sp = comp + (g + from);
                wide_lds8_t dp = outb + ((uint32_t)__builtin_amdgcn_readlane((int)dstp, (int)le) + (from - ps));
                if (n >= 4u) {
                    for (uint32_t i = 4u * lane; i < n; i += 4u * kWave) {
                        const uint32_t o = i < n - 4u ? i : n - 4u;  // the last step clamped back: same bytes, same place
                        wide_st32u(dp + o, wide_ld32u(sp + o));
                    }
                } else if (lane < n) {
                    dp[lane] = sp[lane];
                }
            }
        }
        // ---- copies: where each of their bytes comes from ----
        if (starts && e_type != 0)
            for (uint32_t k = 0; k < e_len; ++k) srcmap[dstp + k] = (uint16_t)(dstp + k - offv);
        op += total;
        cp = g + s;
    }
    landing = cp;
    op_end = op;
    return ok;
}

__global__ __launch_bounds__(1024) void k2_wide_kernel(const uint8_t* stream, uint64_t stream_len, const uint64_t* __restrict__ block_offsets,
                                                        uint64_t total_len, uint32_t block_size, uint8_t* out, uint32_t* __restrict__ status,
                                                        uint32_t num_blocks, uint32_t* result, uint32_t* next_block)
{
    __shared__ __attribute__((aligned(16))) uint8_t wide_mem[kWideLdsBytes];
    wide_lds8_t mem = (wide_lds8_t)wide_mem;
    wide_lds8_t comp = mem + kWideCompAt;
    wide_lds8_t outb = mem + kWideOutAt;
    wide_lds16_t srcmap = (wide_lds16_t)(mem + kWideMapAt);
    wide_lds64_t table = (wide_lds64_t)(mem + kWideTableAt);
    wide_lds32_t ctl = (wide_lds32_t)(mem + kWideCtlAt);
    lds_bytes_t k2_stage = (lds_bytes_t)(wide_mem + kWideTableAt);   // the fallback's stage: the table is done with by then
    const uint32_t tid = threadIdx.x, lane = tid & 63u, threads = blockDim.x, waves = threads >> 6;
    const uint32_t wave = uni(tid >> 6);                             // (an SGPR: the share's bounds feed K2's scalar chain walk)

    for (;;) {
        if (tid == 0) ctl[kWideDrawn] = atomicAdd(next_block, 1u);
        __syncthreads();
        const uint32_t b = uni(ctl[kWideDrawn]);
        if (b >= num_blocks) break;
        const uint64_t at = uld64(reinterpret_cast<const uint8_t*>(block_offsets + b));
        const uint64_t ostart = (uint64_t)b * block_size;
        const uint64_t oleft = total_len - ostart;
        const uint32_t out_len = (oleft < block_size) ? (uint32_t)oleft : block_size;
        uint8_t* win = out + ostart;

        // ---- the limits ----
        bool within = block_size <= kWideMaxBlock && at <= stream_len && stream_len - at >= 4u;    // (out_len <= block_size)
        uint32_t csz = 0;
        if (within) {
            csz = uld32(stream + at);
            within = csz <= kWideMaxCsz && (uint64_t)csz <= stream_len - at - 4u;
        }
        bool proven = false;
        if (within) {
            // ---- A: stage ----
            const uint8_t* src = stream + at + 4u;
            const uint32_t body = csz & ~15u;
            for (uint32_t i = 16u * tid; i < body; i += 16u * threads) {
                const uint4 v = ld128(src + i);
                *reinterpret_cast<wide_lds128_t>(comp + i) = wide_v4_t{v.x, v.y, v.z, v.w};
            }
            if (tid < csz - body) comp[body + tid] = src[body + tid];
            if (tid < 128u) comp[csz + tid] = 0;
            for (uint32_t i = 8u * tid; i < out_len; i += 8u * threads) {
                const uint32_t p = i | ((i + 1u) << 16);
                *reinterpret_cast<wide_lds128_t>(srcmap + i) = wide_v4_t{p, p + 0x00020002u, p + 0x00040004u, p + 0x00060006u};
            }
            if (tid < kWideMaxWaves) ctl[tid] = kWideNone;
            if (tid < 2u + kWideRounds + 2u) ctl[kWideBadC + tid] = 0;
            __syncthreads();
            // ---- B: shares ----
            const uint32_t per = (csz + waves - 1u) / waves;
            const uint32_t share = per > 64u ? (per + 63u) & ~63u : 64u;
            {
                const uint32_t start = wave * share;
                if (start < csz) {
                    const uint32_t end = start + share < csz ? start + share : csz;
                    table[wave * kWideZone + lane] = wide_lane_walk(comp, start + lane, end, csz);
                }
            }
            __syncthreads();
            // ---- C: resolve the true chain ----
            if (tid == 0) {
                uint32_t e = 0, base = 0;
                bool ok = true;
                while (e < csz) {
                    const uint32_t s = e / share;
                    const uint32_t zone = s * share;
                    const uint32_t end = zone + share < csz ? zone + share : csz;
                    const uint64_t t = (e - zone < kWideZone) ? table[s * kWideZone + (e - zone)] : wide_lane_walk(comp, e, end, csz);
                    const uint32_t landing = (uint32_t)t, o = (uint32_t)(t >> 32);
                    if (t == kWideInvalid || o > out_len - base) {
                        ok = false;
                        break;
                    }
                    ctl[s] = e;
                    ctl[16u + s] = base;
                    ctl[32u + s] = landing;
                    ctl[48u + s] = base + o;
                    base += o;
                    e = landing;
                }
                if (!ok || e != csz || base != out_len) ctl[kWideBadC] = 1;
            }
            __syncthreads();
            // ---- D: mark and place ----
            if (ctl[kWideBadC] == 0) {
                const uint32_t entry = uni(ctl[wave]);
                if (entry != kWideNone) {
                    const uint32_t start = wave * share;
                    const uint32_t limit = start + share < csz ? start + share : csz;
                    const uint32_t base = uni(ctl[16u + wave]), want_landing = uni(ctl[32u + wave]), want_end = uni(ctl[48u + wave]);
                    uint32_t landing = 0, op_end = 0;
                    // (the entry is step C's own; tested all the same, so that no word of the table can send a load out of the stage)
                    const bool ok = entry >= start && entry < limit && base <= out_len &&
                                    wide_share_walk(comp, csz, entry, limit, base, out_len, outb, srcmap, lane, landing, op_end);
                    if ((!ok || landing != want_landing || op_end != want_end) && lane == 0) ctl[kWideBadD] = 1;
                }
            }
            __syncthreads();
            proven = ctl[kWideBadC] == 0 && ctl[kWideBadD] == 0;
            if (proven) {
                // ---- E: resolve copies by pointer doubling (a thread owns its four entries; others only read them, and any
                //      value they can see there is an ancestor of the entry: the rounds need no second barrier) ----
                bool settled = false;
                for (uint32_t r = 0; r < kWideRounds; ++r) {
                    bool changed = false;
                    for (uint32_t i = 4u * tid; i < out_len; i += 4u * threads) {
                        const uint64_t q = *reinterpret_cast<wide_lds64_t>(srcmap + i);
                        const uint32_t s0 = (uint32_t)q & 0xffffu, s1 = (uint32_t)(q >> 16) & 0xffffu, s2 = (uint32_t)(q >> 32) & 0xffffu,
                                       s3 = (uint32_t)(q >> 48);
                        const uint64_t n = (uint64_t)srcmap[s0] | ((uint64_t)srcmap[s1] << 16) | ((uint64_t)srcmap[s2] << 32) |
                                           ((uint64_t)srcmap[s3] << 48);
                        if (n != q) {
                            *reinterpret_cast<wide_lds64_t>(srcmap + i) = n;
                            changed = true;
                        }
                    }
                    if (changed) ctl[kWideChanged + r] = 1;
                    __syncthreads();
                    if (ctl[kWideChanged + r] == 0) {
                        settled = true;
                        break;
                    }
                }
                proven = settled;                                    // (it always is: srcmap[i] <= i, the chains end)
            }
            if (proven) {
                for (uint32_t i = tid; i < out_len; i += threads) {
                    const uint32_t s = srcmap[i];
                    if (s != i) outb[i] = outb[s];                   // (s is a literal's byte: nobody writes it here)
                }
                __syncthreads();
                // ---- F: store ----
                const uint32_t head = (uint32_t)((16 - ((uintptr_t)win & 15)) & 15);
                const uint32_t h = head < out_len ? head : out_len;
                if (tid < h) win[tid] = outb[tid];
                const uint32_t mid = (out_len - h) & ~15u;
                for (uint32_t i = 16u * tid; i < mid; i += 16u * threads)
                    *reinterpret_cast<wide_v4_t*>(win + h + i) = *reinterpret_cast<SNAPPY_WIDE_LDS const wide_u128_unaligned_t*>(outb + h + i);
                const uint32_t done = h + mid;
                if (done + tid < out_len) win[done + tid] = outb[done + tid];
                if (tid == 0) {
                    status[b] = kBlockOk;
                    atomicAdd(result + 0, 1u);
                }
            }
        }
        // ---- the serial decoder: K2's own, for what is beyond the limits and what was not proven ----
        if (!proven && wave == 0) {
            const uint32_t st = k2_decode_block<false>(stream, stream_len, at, win, out_len, k2_stage);
            if (lane == 0) {
                status[b] = st;
                atomicAdd(result + (within ? 2 : 1), 1u);
            }
        }
        __syncthreads();            // (the control words and the stage belong to this trip until here)
    }
}

}  // namespace snappy_hip
