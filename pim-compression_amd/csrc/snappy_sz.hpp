// snappy_sz.hpp -- the Snappy FRAMING format (.sz: what snzip, Go's snappy.Writer and snappy-java's framed streams write) on the
// device: snappy_hip_sz_decompress_batch and snappy_hip_sz_compress_batch (include/snappy_hip.h).
//
// A stream is a chain of chunks: a type byte, a 3-byte little-endian length L, L bytes.  0xff = the identifier ("sNaPpY",
// first, may repeat), 0x00 = masked CRC-32C of the plaintext + one raw Snappy stream of at most 65536 bytes, 0x01 = masked
// CRC + plain bytes, 0x80..0xfe skipped, 0x02..0x7f refused.  An item is a RawItem (src, src_len, dst, dst_capacity).
//   * decode: sz_index_kernel<false> (a wavefront per stream walks the chain: verdict, length, number of data chunks),
//     sz_plan_kernel (one workgroup: the chunks' prefix over the items, the max_chunks cut), sz_index_kernel<true> (the same
//     walk again, now with a place to record every data chunk; item 0, whose place is known from the start, is recorded by
//     the first walk), sz_decode_chunks_kernel (persistent wavefronts, one counter: a chunk is decoded by k2_decode_block<true>
//     or copied, then read back and its CRC compared -- the same wavefront, behind stores_landed(), as K2's far copies read
//     what the wavefront wrote) and sz_finish_kernel (a wavefront per item: the lowest-numbered bad chunk).  The other chains
//     are walked twice because a chunk's record needs its number in the batch, which needs every earlier item's count.
//   * compress: a CHUNK is chunk_len bytes of an item compressed as one K1 block, the raw compress's pipeline
//     (snappy_raw.hpp) with a CRC kernel of its own and a sizes step that picks each chunk's type: sz_compress_plan_kernel,
//     sz_compress_chunks_kernel, sz_chunk_crc_kernel, sz_sizes_kernel, sz_gather_kernel.
// Every kernel here is new; k2_decode_block, LDS_TABLE_WAVE_COMPRESS and the pieces of snappy_device_common.hpp are used as
// they are.
#pragma once
#include "snappy_crc32c.hpp"
#include "snappy_raw.hpp"      // RawItem, the raw statuses, kRawMaxLen, k2_decode_block, LdsTableWave

namespace snappy_hip {

constexpr uint32_t kSzCrcMismatch = 7;       // SNAPPY_HIP_SZ_CRC_MISMATCH
constexpr uint32_t kSzUnsupported = 8;       // SNAPPY_HIP_SZ_UNSUPPORTED
constexpr uint32_t kSzNoVerify = 1;          // SNAPPY_HIP_SZ_NO_VERIFY
constexpr uint32_t kSzMaxChunk = 65536;      // the most plaintext one chunk holds
constexpr uint32_t kSzIdentifierBytes = 10;

enum : uint32_t { kSzCtlChunks = 0 };        // word of the control line: the chunks to decode / compress

// one data chunk of a stream being decoded
struct SzChunk {
    uint64_t src_off;          // of the chunk's type byte in its item's src
    uint64_t dst_off;          // of its plaintext in its item's dst
    uint32_t info;             // L | length of the varint << 24 | (type 0x00) << 28
    uint32_t ulen;             // uncompressed length
    uint32_t item;
    uint32_t status;
};
constexpr uint32_t kSzInfoCompressed = 1u << 28;

// Scratch of one decode call, every part rounded up to 256 bytes: control line, prefix[count + 1] (u64: first chunk of item
// i; [count] = all chunks), chunks[max_chunks].
struct SzDecodeLayout {
    uint64_t prefix, chunks, total;
};
__host__ __device__ inline SzDecodeLayout sz_decode_layout(uint32_t count, uint32_t max_chunks)
{
    SzDecodeLayout l;
    l.prefix = 256;
    l.chunks = l.prefix + round256(((uint64_t)count + 1u) * 8u);
    l.total = l.chunks + round256((uint64_t)max_chunks * sizeof(SzChunk));
    return l;
}

// The walk of one stream's chunk chain, by every lane of a wavefront alike (src, src_len wave-uniform, src_len <= kRawMaxLen):
// the verdict of the chain, the number of data chunks and the sum of their uncompressed lengths.  kRecord: lane 0 writes
// chunk k's record to rec[k] (its dst_off is the sum so far) while k < limit.
// The walk is a chain of dependent loads, about 0.95 us per chunk on an MI355X: the miss on the next header.  (Taking the header
// and the varint in one 16-byte load did not change that, measured, and is not kept.)
template <bool kRecord>
__device__ __forceinline__ uint32_t sz_walk(const uint8_t* src, uint64_t src_len, uint64_t& total_out, uint32_t& chunks_out, SzChunk* rec,
                                            uint32_t limit, uint32_t item, uint32_t lane)
{
    uint64_t at = 0, total = 0;
    uint32_t chunks = 0, st = kBlockOk;
    bool identified = false;
    while (at < src_len) {
        if (at + 4 > src_len) {
            st = kBlockInvalid;
            break;
        }
        const uint32_t w = uld32(src + at);
        const uint32_t type = w & 0xffu, L = w >> 8;
        if (at + 4 + L > src_len) {                                  // a chunk running past the stream
            st = kBlockInvalid;
            break;
        }
        if (type == 0xffu) {
            // "sNaPpY"
            if (L != 6 || uld32(src + at + 4) != 0x50614e73u || uni((uint32_t)src[at + 8]) != 0x70u || uni((uint32_t)src[at + 9]) != 0x59u) {
                st = kBlockInvalid;
                break;
            }
            identified = true;
        } else if (!identified) {                                    // the first chunk is not the identifier
            st = kBlockInvalid;
            break;
        } else if (type <= 1u) {
            if (L < 4) {
                st = kBlockInvalid;
                break;
            }
            uint32_t length = L - 4, hdr = 0;
            if (type == 0) {
                // the raw stream's header, by the rules of SNAPPY_RAW_ITEM_VERDICT: at most 5 bytes, the fifth below 16, inside
                // the chunk
                length = 0;
                for (uint32_t k = 0; k < 5 && k < L - 4; ++k) {
                    const uint32_t c = uni((uint32_t)src[at + 8 + k]);
                    if (k == 4 && c >= 16u) break;
                    length |= (c & 0x7fu) << (7u * k);
                    if (c < 0x80u) {
                        hdr = k + 1;
                        break;
                    }
                }
                if (hdr == 0) {
                    st = kBlockInvalid;
                    break;
                }
            }
            if (length > kSzMaxChunk) {                              // an oversized chunk
                st = kBlockInvalid;
                break;
            }
            if (kRecord && lane == 0 && chunks < limit) {
                SzChunk c;
                c.src_off = at;
                c.dst_off = total;
                c.info = L | (hdr << 24) | (type == 0 ? kSzInfoCompressed : 0u);
                c.ulen = length;
                c.item = item;
                c.status = kBlockOk;
                rec[chunks] = c;
            }
            total += length;
            ++chunks;
        } else if (type < 0x80u) {                                   // reserved unskippable
            st = kSzUnsupported;
            break;
        }                                                            // (0x80..0xfe: skipped)
        at += 4ull + L;
    }
    if (st == kBlockOk && !identified) st = kBlockInvalid;          // no identifier: an empty stream
    total_out = total;
    chunks_out = chunks;
    return st;
}

// SNAPPY_SZ_NO_KERNELS: a second source of the library that needs SzChunk, sz_walk and the layout (snappy_hip_sz_split.hip, the
// split walk of snappy_sz_split.hpp) takes this header without its kernels: two of them are no templates and would be defined twice.
#ifndef SNAPPY_SZ_NO_KERNELS

// One wavefront per item.  kRecord = false: status[i], out_len[i] (the total length whenever the chain parses) and prefix[i] =
// the item's number of data chunks (0 unless it is OK).  kRecord = true, behind sz_plan_kernel: the chunks of the items still
// OK are recorded at chunks[prefix[i]..].  Item 0's first chunk is chunk 0 of the batch whatever the plan finds, so the first
// walk records it already (the first max_chunks of its chunks; the plan refuses it if there are more) and the second passes it
// by: a call with ONE stream, what the one-buffer calls make, walks its chain once.
template <bool kRecord>
__global__ __launch_bounds__(64) void sz_index_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t max_chunks,
                                                      uint64_t* __restrict__ out_len, uint32_t* __restrict__ status, uint64_t* __restrict__ prefix,
                                                      SzChunk* __restrict__ chunks)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        if (kRecord && (i == 0 || uni(status[i]) != kBlockOk)) continue;
        const uint8_t* src = load_global_ptr(&items[i].src);
        uint8_t* dst = load_global_ptr(&items[i].dst);
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
        const uint64_t capacity = dst ? uld64(reinterpret_cast<const uint8_t*>(&items[i].dst_capacity)) : 0;
        uint64_t total = 0;
        uint32_t n = 0, st;
        if (!src) {
            st = kBlockInvalid;
        } else if (src_len > kRawMaxLen) {
            st = kRawTooLarge;
        } else {
            if (kRecord) st = sz_walk<true>(src, src_len, total, n, chunks + uld64(reinterpret_cast<const uint8_t*>(prefix + i)), 0xffffffffu, i, lane);
            else if (i == 0) st = sz_walk<true>(src, src_len, total, n, chunks, max_chunks, i, lane);
            else st = sz_walk<false>(src, src_len, total, n, nullptr, 0, i, lane);
            if (st != kBlockOk) total = 0;
            else if (total > kRawMaxLen) st = kRawTooLarge;
            else if (total > capacity) st = kRawDstTooSmall;
        }
        if (!kRecord && lane == 0) {
            status[i] = st;
            out_len[i] = total;
            prefix[i] = st == kBlockOk ? n : 0u;
        }
    }
}

// One workgroup: prefix[] from the items' chunk counts to their exclusive prefix; the items whose chunks lie beyond max_chunks
// are RAW_TOO_LARGE; result[0] = the chunks the batch needs, result[1] = 0 (sz_finish_kernel counts into it).
__global__ __launch_bounds__(1024) void sz_plan_kernel(uint32_t count, uint32_t max_chunks, uint32_t* __restrict__ status,
                                                       uint32_t* __restrict__ result, uint32_t* __restrict__ ctl, uint64_t* __restrict__ prefix)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint64_t cut_s;
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < count; base += 1024) {
        const uint32_t i = base + tid;
        const uint64_t mine = i < count ? prefix[i] : 0;
        uint64_t total;
        const uint64_t first = carry + workgroup_exclusive_scan(mine, wave_sums, total);
        if (i < count) {
            prefix[i] = first;
            const bool beyond = mine && first + mine > max_chunks;
            if (beyond && first <= max_chunks) cut_s = first;
            if (beyond) status[i] = kRawTooLarge;
        }
        carry += total;
    }
    __syncthreads();
    if (tid == 0) {
        prefix[count] = carry;
        ctl[kSzCtlChunks] = (uint32_t)(carry > max_chunks ? cut_s : carry);
        result[0] = carry > 0xffffffffull ? 0xffffffffu : (uint32_t)carry;
        result[1] = 0;
    }
}

// Persistent wavefronts draw chunk numbers.  flags: kSzNoVerify skips the CRC.
// amdgpu_num_sgpr: as on decompress_blocks_kernel (snappy_kernels.hpp) -- the 80 scalar registers this kernel took before
// k2_decode_block had two window loops; it would take 81 now.
template <int kTables>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_sgpr(80))) void sz_decode_chunks_kernel(const RawItem* __restrict__ items, const uint32_t* __restrict__ ctl,
                                                              SzChunk* __restrict__ chunks, uint32_t flags, uint32_t* next_chunk)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage_mem[kK2StageBytes];   // one window's output (K2's stage)
    __shared__ uint32_t table[crc_table_words<kTables>()];
    lds_bytes_t stage = (lds_bytes_t)stage_mem;
    const uint32_t lane = threadIdx.x;
    crc_table_init<kTables>(table, lane);
    __syncthreads();
    const uint32_t total = uni(ctl[kSzCtlChunks]);

    for (;;) {
        const uint32_t c = draw_work(next_chunk, lane);
        if (c >= total) break;
        const uint8_t* rec = reinterpret_cast<const uint8_t*>(chunks + c);
        const uint64_t src_off = uld64(rec), dst_off = uld64(rec + 8);
        const uint32_t info = uld32(rec + 16), ulen = uld32(rec + 20), i = uld32(rec + 24);
        const uint8_t* src = load_global_ptr(&items[i].src) + src_off;
        uint8_t* dst = load_global_ptr(&items[i].dst) + dst_off;
        const uint32_t payload = (info & 0xffffffu) - 4u, hdr = (info >> 24) & 7u;
        uint32_t st = kBlockOk;
        if (info & kSzInfoCompressed) {
            if (ulen == 0) st = payload == hdr ? kBlockOk : kBlockInvalid;      // nothing may follow the header
            else st = k2_decode_block<true>(src + 8, payload, hdr, dst, ulen, stage);
        } else {
            wave_copy(dst, src + 8, ulen, lane);
        }
        if (st == kBlockOk && !(flags & kSzNoVerify)) {
            stores_landed();
            const uint32_t crc = ~crc32c_wave<kTables>(0xffffffffu, dst, ulen, lane, table);
            if (crc_mask(crc) != uld32(src + 4)) st = kSzCrcMismatch;
        }
        if (lane == 0) chunks[c].status = st;
        __syncthreads();
    }
}

// One wavefront per item still OK: status[i] = the status of its lowest-numbered bad chunk, bad_chunk[i] = that chunk's
// number in the item (0xffffffff: none); result[1] counts the items that are OK.
__global__ __launch_bounds__(64) void sz_finish_kernel(uint32_t count, const uint64_t* __restrict__ prefix, const SzChunk* __restrict__ chunks,
                                                       uint32_t* __restrict__ status, uint32_t* __restrict__ bad_chunk, uint32_t* __restrict__ result)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        uint32_t st = uni(status[i]), bad = 0xffffffffu;
        if (st == kBlockOk) {
            const uint64_t first = uld64(reinterpret_cast<const uint8_t*>(prefix + i)), end = uld64(reinterpret_cast<const uint8_t*>(prefix + i + 1));
            for (uint64_t base = first; base < end && st == kBlockOk; base += kWave) {
                const uint64_t f = base + lane;
                const uint32_t mine = f < end ? chunks[f].status : kBlockOk;
                const unsigned long long any = __ballot(mine != kBlockOk);
                if (any) {
                    const uint32_t at = (uint32_t)__builtin_ctzll(any);
                    st = (uint32_t)__builtin_amdgcn_readlane((int)mine, at);
                    bad = (uint32_t)(base - first) + at;
                }
            }
        }
        if (lane == 0) {
            status[i] = st;
            bad_chunk[i] = bad;
            if (st == kBlockOk) atomicAdd(result + 1, 1u);
        }
    }
}

// ---- compress ----
// Scratch of one compress call: the raw compress's (control line, prefix, frag_bytes, place, slots) with the chunks' masked
// CRC words in front of the slots.  place[f]: the chunk's offset in its item's dst, bit 63 = it is written compressed.
struct SzCompressLayout {
    uint64_t prefix, frag_bytes, place, crc, slots, total;
};
__host__ __device__ inline SzCompressLayout sz_compress_layout(uint32_t count, uint32_t max_chunks, uint32_t slot_stride)
{
    SzCompressLayout l;
    l.prefix = 256;
    l.frag_bytes = l.prefix + round256(((uint64_t)count + 1u) * 8u);
    l.place = l.frag_bytes + round256((uint64_t)max_chunks * 4u);
    l.crc = l.place + round256((uint64_t)max_chunks * 8u);
    l.slots = l.crc + round256((uint64_t)max_chunks * 4u);
    l.total = l.slots + round256((uint64_t)max_chunks * slot_stride);
    return l;
}
constexpr uint64_t kSzPlaceCompressed = 1ull << 63;

// raw_plan_kernel's plan with chunks for fragments
__global__ __launch_bounds__(1024) void sz_compress_plan_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t chunk_len,
                                                                uint32_t max_chunks, uint64_t* __restrict__ out_len, uint32_t* __restrict__ status,
                                                                uint32_t* __restrict__ result, uint32_t* __restrict__ ctl,
                                                                uint64_t* __restrict__ prefix)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint64_t cut_s;
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < count; base += 1024) {
        const uint32_t i = base + tid;
        uint64_t mine = 0;
        uint32_t st = kBlockOk;
        if (i < count) {
            const RawItem q = items[i];
            if (q.src_len >> 32) st = kRawTooLarge;
            else if (q.src_len && !q.src) st = kBlockInvalid;
            else mine = (q.src_len + chunk_len - 1) / chunk_len;
        }
        uint64_t total;
        const uint64_t first = carry + workgroup_exclusive_scan(mine, wave_sums, total);
        if (i < count) {
            prefix[i] = first;
            const bool beyond = mine && first + mine > max_chunks;
            if (beyond && first <= max_chunks) cut_s = first;
            status[i] = beyond ? kRawTooLarge : st;
            out_len[i] = 0;
        }
        carry += total;
    }
    __syncthreads();
    if (tid == 0) {
        prefix[count] = carry;
        ctl[kSzCtlChunks] = (uint32_t)(carry > max_chunks ? cut_s : carry);
        result[0] = carry > 0xffffffffull ? 0xffffffffu : (uint32_t)carry;
        result[1] = 0;
    }
}

// raw_compress_fragments_kernel's trip: chunk f as one K1 block into slot f
template <int kForm>
__global__ __launch_bounds__(64) void sz_compress_chunks_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t chunk_len,
                                                                const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ prefix,
                                                                uint32_t* __restrict__ frag_bytes, uint8_t* __restrict__ slots, uint32_t slot_stride,
                                                                uint32_t* next_chunk)
{
    HIP_DYNAMIC_SHARED(uint8_t, lds_dyn)
    const LdsTableWave k1(lds_dyn, chunk_len);
    const uint32_t lane = threadIdx.x;
    const uint32_t chunks = uni(ctl[kSzCtlChunks]);

    for (;;) {
        const uint32_t f = draw_work(next_chunk, lane);
        if (f >= chunks) break;
        const uint32_t i = prefix_owner<false>(prefix, count, f);
        const uint8_t* src = load_global_ptr(&items[i].src);
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));   // (validated: < 4 GiB)
        const uint64_t start = (f - uld64(reinterpret_cast<const uint8_t*>(prefix + i))) * chunk_len;
        const uint64_t left = src_len - start;
        const uint32_t n = left < chunk_len ? (uint32_t)left : chunk_len;
        uint8_t* out = slots + (uint64_t)f * slot_stride;
        LDS_TABLE_WAVE_COMPRESS(kForm, k1, src, start, src_len, n, out, lane, frag_bytes + f);
        __syncthreads();
    }
}

// Persistent wavefronts draw chunk numbers: crc[f] = the masked CRC-32C of chunk f's plaintext.  Independent of the parse.
template <int kTables>
__global__ __launch_bounds__(64) void sz_chunk_crc_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t chunk_len,
                                                          const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ prefix,
                                                          uint32_t* __restrict__ crc, uint32_t* next_chunk)
{
    __shared__ uint32_t table[crc_table_words<kTables>()];
    const uint32_t lane = threadIdx.x;
    crc_table_init<kTables>(table, lane);
    __syncthreads();
    const uint32_t chunks = uni(ctl[kSzCtlChunks]);
    for (;;) {
        const uint32_t f = draw_work(next_chunk, lane);
        if (f >= chunks) break;
        const uint32_t i = prefix_owner<true>(prefix, count, f);
        const uint8_t* src = load_global_ptr(&items[i].src);
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
        const uint64_t start = (f - uld64(reinterpret_cast<const uint8_t*>(prefix + i))) * chunk_len;
        const uint64_t left = src_len - start;
        const uint32_t n = left < chunk_len ? (uint32_t)left : chunk_len;
        const uint32_t c = ~crc32c_wave<kTables>(0xffffffffu, src + start, n, lane, table);
        if (lane == 0) crc[f] = crc_mask(c);
        __builtin_amdgcn_wave_barrier();
    }
}

// One wavefront per item the plan left OK: each chunk's type (compressed iff varint + elements are shorter than the plaintext)
// and size, scanned into its place behind the identifier; an item that does not fit its dst is told the size it needs and
// keeps every byte of dst.
__global__ __launch_bounds__(64) void sz_sizes_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t chunk_len,
                                                      const uint64_t* __restrict__ prefix, const uint32_t* __restrict__ frag_bytes,
                                                      uint64_t* __restrict__ place, uint64_t* __restrict__ out_len, uint32_t* __restrict__ status,
                                                      uint32_t* __restrict__ result)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        if (uni(status[i]) != kBlockOk) continue;
        const uint64_t first = uld64(reinterpret_cast<const uint8_t*>(prefix + i)), end = uld64(reinterpret_cast<const uint8_t*>(prefix + i + 1));
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
        uint64_t at = kSzIdentifierBytes;
        for (uint64_t base = first; base < end; base += kWave) {
            const uint64_t f = base + lane;
            uint32_t mine = 0;
            bool compressed = false;
            if (f < end) {
                const uint64_t left = src_len - (f - first) * chunk_len;
                const uint32_t n = left < chunk_len ? (uint32_t)left : chunk_len;
                const uint32_t raw = varint32_len(n) + frag_bytes[f] - 4u;
                compressed = raw < n;
                mine = 8u + (compressed ? raw : n);
            }
            const uint32_t x = wave_inclusive_scan(mine, lane);
            if (f < end) place[f] = (at + (x - mine)) | (compressed ? kSzPlaceCompressed : 0ull);
            at += (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
        }
        uint8_t* dst = load_global_ptr(&items[i].dst);
        const uint64_t capacity = dst ? uld64(reinterpret_cast<const uint8_t*>(&items[i].dst_capacity)) : 0;
        if (lane == 0) {
            out_len[i] = at;
            if (at > capacity) {
                status[i] = kRawDstTooSmall;
            } else {
                const uint8_t id[kSzIdentifierBytes] = {0xff, 6, 0, 0, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};
                for (uint32_t k = 0; k < kSzIdentifierBytes; ++k) dst[k] = id[k];
                atomicAdd(result + 1, 1u);
            }
        }
    }
}

// One 256-thread workgroup per chunk: the header, the CRC word and the payload -- the varint and the slot's elements for a
// compressed chunk, the plaintext from src for an uncompressed one; both ends at any alignment (workgroup_copy).
__global__ __launch_bounds__(256) void sz_gather_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t chunk_len,
                                                        const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ prefix,
                                                        const uint32_t* __restrict__ frag_bytes, const uint64_t* __restrict__ place,
                                                        const uint32_t* __restrict__ crc, const uint8_t* __restrict__ slots, uint32_t slot_stride,
                                                        const uint32_t* __restrict__ status)
{
    const uint32_t chunks = ctl[kSzCtlChunks];
    for (uint32_t f = blockIdx.x; f < chunks; f += gridDim.x) {
        const uint32_t i = prefix_owner<false>(prefix, count, f);
        if (status[i] != kBlockOk) continue;
        const uint8_t* src = load_global_ptr(&items[i].src);
        const uint64_t start = (f - prefix[i]) * chunk_len;
        const uint64_t left = items[i].src_len - start;
        const uint32_t n = left < chunk_len ? (uint32_t)left : chunk_len;
        const uint64_t pl = place[f];
        const bool compressed = (pl & kSzPlaceCompressed) != 0;
        uint8_t* dst = load_global_ptr(&items[i].dst) + (pl & ~kSzPlaceCompressed);
        const uint32_t elements = frag_bytes[f] - 4u;
        const uint32_t vlen = compressed ? varint32_len(n) : 0u;
        if (threadIdx.x == 0) {
            const uint32_t L = 4u + (compressed ? vlen + elements : n);
            dst[0] = compressed ? 0x00 : 0x01;
            dst[1] = (uint8_t)L;
            dst[2] = (uint8_t)(L >> 8);
            dst[3] = (uint8_t)(L >> 16);
            const uint32_t c = crc[f];
            dst[4] = (uint8_t)c;
            dst[5] = (uint8_t)(c >> 8);
            dst[6] = (uint8_t)(c >> 16);
            dst[7] = (uint8_t)(c >> 24);
            if (compressed) put_varint32(dst + 8, n);
        }
        if (compressed) workgroup_copy(dst + 8 + vlen, slots + (uint64_t)f * slot_stride + 4, elements);
        else workgroup_copy(dst + 8, src + start, n);
    }
}

#endif  // SNAPPY_SZ_NO_KERNELS

}  // namespace snappy_hip
