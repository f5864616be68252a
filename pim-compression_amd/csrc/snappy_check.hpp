// snappy_check.hpp -- containers and raw streams checked on the device without being decoded (snappy_hip_check_blocks,
// snappy_hip_raw_check_batch, include/snappy_hip.h).
//
// A block's verdict in k2_decode_block (snappy_kernels.hpp) depends on the stream's bytes alone: an element predecode
// rejected on the chain, `op + total > out_len`, a copy with a zero offset or one that reaches before the block's first
// output byte, `op != out_len || cp != csz` at the end, and the two bounds of the size word.  None of them reads a byte of
// output.  k2_check_block runs K2's window loop with everything that produces output taken out -- no output buffer, no LDS
// stage, no far-copy loads, no store but the verdict -- and gives exactly K2's verdict.  It has a loop skeleton of its own
// (K2's code must not change by a single instruction); tests/test_check_emulated.py and tests/test_gpu_check.py hold the two
// to each other block for block.  Three kernels:
//   * check_plan_kernel (one workgroup, the planner loop of range_pieces_kernel): validates every descriptor, initialises its
//     four result words and writes the exclusive prefix of the containers' block counts;
//   * check_kernel (persistent wavefronts, one counter, as K2): a wavefront draws a global block number, finds its container
//     by a binary search over the prefix and checks the block;
//   * raw_check_kernel: items drawn as raw_decompress_kernel draws them, the same header rules, k2_check_block<true>.
// It checks ELEMENTS, not links: a block is read at the offset the descriptor gives, as K2 reads it.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_kernels.hpp"   // window_issue, predecode_window, k2_chain_walk, StreamDesc
#include "snappy_raw.hpp"       // RawItem, kRawMaxLen, kRawTooLarge

namespace snappy_hip {

constexpr uint64_t kMaxCheckBlocks = 1ull << 31;    // blocks one call checks at most (the work counter is 32 bits)
constexpr uint32_t kCheckNone = 0xffffffffu;        // "no invalid block" in a container's third result word

// Scratch of one call: the block prefix (count + 2 u64: [i] = first global block of container i, [count] = all blocks,
// [count + 1] = blocks to check), rounded up to 256 bytes.
__host__ __device__ inline uint64_t check_prefix_bytes(uint32_t count) { return round256(((uint64_t)count + 2u) * 8u); }

// K2's verdict on ONE block without decoding it: the block whose u32 size prefix is at stream + at, for an output of out_len
// bytes.  Returns kBlockOk / kBlockInvalid.  Wave-uniform arguments; every lane of the wavefront calls it.  kRaw as in
// k2_decode_block: one raw Snappy stream, the elements are stream[at, stream_len).
// The cursors are K2's: g = window base, cp / op = compressed / output cursor, the window registers rotate at the end of a
// window, and a literal that runs on beyond the two prefetched windows (cp >= g + 128) makes the next window load afresh --
// which is all that skipping a long literal costs here.
template <bool kRaw = false>
__device__ __forceinline__ uint32_t k2_check_block(const uint8_t* stream, uint64_t stream_len, uint64_t at, uint32_t out_len)
{
    const uint32_t lane = threadIdx.x;
    uint32_t st = kBlockOk;
    uint32_t csz = 0;
    if constexpr (kRaw) {
        csz = (uint32_t)(stream_len - at);                           // (the caller has checked at <= stream_len <= kRawMaxLen)
    } else if (at + 4 > stream_len) {
        st = kBlockInvalid;
    } else {
        csz = uld32(stream + at);
        if (at + 4 + (uint64_t)csz > stream_len) st = kBlockInvalid;
    }
    const uint32_t skip = kRaw ? 0u : 4u;
    const uint8_t* __restrict__ src = stream + at + skip;
    const uint64_t avail = (st == kBlockOk) ? stream_len - (at + skip) : 0;

    uint32_t g = 0;
    uint32_t cp = 0, op = 0;
    uint64_t w0 = 0;
    WindowLoad next = {0, 64};
    WindowLoad next2 = {0, 64};
    bool have_window = false;
    const uint32_t avail32 = avail > 0xffffff00ull ? 0xffffff00u : (uint32_t)avail;
    bool next_tail = true, next2_tail = true;
    auto issue = [&](uint32_t base, bool& tail) -> WindowLoad {
        WindowLoad r;
        if (base + 72u <= avail32) {
            r.raw = ld64(src + (base + lane));
            r.shift = 0;
            tail = false;
        } else {
            r = window_issue(src, (uint64_t)base + lane, avail);
            tail = true;
        }
        return r;
    };
    while (st == kBlockOk && cp < csz) {                             // one iteration per 64-byte window
        if (!have_window) {
            g = cp & ~63u;
            bool cur_tail;
            const WindowLoad cur = issue(g, cur_tail);
            next = issue(g + 64u, next_tail);
            next2 = issue(g + 128u, next2_tail);
            w0 = cur_tail ? window_value(cur) : cur.raw;
            have_window = true;
        }
        const uint32_t wend = (csz < g + 64) ? csz : g + 64;
        const uint32_t wlim = wend - g;
        uint32_t e_type, e_hdr, e_len, e_consumed, offv;
        unsigned long long REJ;
        predecode_window<kRaw>(w0, g + lane, csz, e_type, e_hdr, e_len, offv, e_consumed, REJ);
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
            st = kBlockInvalid;
            break;
        }
        const uint32_t mylen = __builtin_amdgcn_inverse_ballot_w64(E) ? e_len : 0u;
        const uint32_t incl = wave_inclusive_scan(mylen, lane);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t dstp = op + (incl - mylen);                   // where this lane's element would start in the block's output
        const unsigned long long COPY = E & __ballot(e_type != 0);
        if (op + total > out_len || (COPY & (__ballot(offv == 0) | __ballot(offv > dstp)))) {
            st = kBlockInvalid;
            break;
        }
        op += total;
        cp = g + s;
        if (cp < g + 128u) {
            SNAPPY_PIN(next.raw);
            SNAPPY_PIN(next2.raw);
            w0 = next_tail ? window_value(next) : next.raw;
            next = next2;
            next_tail = next2_tail;
            g += 64;
            next2 = issue(g + 128u, next2_tail);
        } else {
            have_window = false;                                     // a long literal: skipped, its payload is never loaded
        }
    }
    if (st == kBlockOk && (op != out_len || cp != csz)) st = kBlockInvalid;
    return st;
}

// Blocks of one container, or ~0 for a malformed descriptor: a block size of 0 or above 65535, a num_blocks that is not
// ceil(total_len / block_size), no block offsets with blocks present, no stream with stream_len > 0.
__device__ __forceinline__ uint64_t check_blocks_of(const StreamDesc& d)
{
    if (d.block_size == 0 || d.block_size > 65535u) return ~0ull;
    const uint64_t nb = ((uint64_t)d.total_len + d.block_size - 1) / d.block_size;
    if (d.num_blocks != nb) return ~0ull;
    if (nb && d.block_offsets == nullptr) return ~0ull;
    if (d.stream_len && d.stream == nullptr) return ~0ull;
    return nb;
}

// One item checked by ONE wavefront, verdict and length stored: a trip of raw_check_kernel and of the split check's serial step
// (snappy_raw_check_split.hpp).  i is wave-uniform; every lane of the wavefront runs it.  A macro for SNAPPY_RAW_ITEM_VERDICT's
// reason: raw_check_kernel's generated code stays what it was.
#define SNAPPY_RAW_CHECK_ITEM(items, i, out_len, status, lane)                                                                    \
    const uint8_t* src = load_global_ptr(&items[i].src);                                                                          \
    const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));                                          \
    /* the header, by raw_decompress_kernel's rule: at most 5 bytes, the fifth below 16, inside the stream */                     \
    uint32_t length = 0, hdr = 0;                                                                                                 \
    if (src)                                                                                                                      \
        for (uint32_t k = 0; k < 5 && k < src_len; ++k) {                                                                         \
            const uint32_t c = uni((uint32_t)src[k]);                                                                             \
            if (k == 4 && c >= 16u) break;                                                                                        \
            length |= (c & 0x7fu) << (7u * k);                                                                                    \
            if (c < 0x80u) {                                                                                                      \
                hdr = k + 1;                                                                                                      \
                break;                                                                                                            \
            }                                                                                                                     \
        }                                                                                                                         \
    uint32_t st;                                                                                                                  \
    if (hdr == 0) {                                                                                                               \
        st = kBlockInvalid;                                                                                                       \
        length = 0;                                                                                                               \
    } else if (src_len > kRawMaxLen || length > kRawMaxLen) {                                                                     \
        st = kRawTooLarge;                                                                                                        \
    } else if (length == 0) {                                                                                                     \
        st = src_len == hdr ? kBlockOk : kBlockInvalid;          /* nothing may follow the header */                              \
    } else {                                                                                                                      \
        st = k2_check_block<true>(src, src_len, hdr, length);                                                                     \
    }                                                                                                                             \
    if (lane == 0) {                                                                                                              \
        status[i] = st;                                                                                                           \
        out_len[i] = length;                                                                                                      \
    }

#ifndef SNAPPY_HIP_NO_KERNELS
__global__ __launch_bounds__(1024) void check_plan_kernel(const StreamDesc* __restrict__ descs, uint32_t count, uint32_t* __restrict__ results,
                                                          uint64_t* __restrict__ prefix)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint64_t cut_s;      // blocks to check when there are more than kMaxCheckBlocks
    const uint32_t tid = threadIdx.x;

    uint64_t carry = 0;
    for (uint32_t base = 0; base < count; base += 1024) {
        const uint32_t i = base + tid;
        uint64_t mine = 0;
        bool bad = false;
        if (i < count) {
            const uint64_t n = check_blocks_of(descs[i]);
            bad = n == ~0ull;
            mine = bad ? 0 : n;
        }
        uint64_t total;
        const uint64_t first = carry + workgroup_exclusive_scan(mine, wave_sums, total);
        if (i < count) {
            prefix[i] = first;
            // past kMaxCheckBlocks: the container that straddles it (exactly one when there are more blocks) marks the cut
            const bool beyond = first + mine > kMaxCheckBlocks;
            if (beyond && first <= kMaxCheckBlocks) cut_s = first;
            results[4 * (uint64_t)i] = (bad || beyond) ? kRangeOutOfBounds : kBlockOk;
            results[4 * (uint64_t)i + 1] = 0;
            results[4 * (uint64_t)i + 2] = kCheckNone;
            results[4 * (uint64_t)i + 3] = 0;
        }
        carry += total;
    }
    __syncthreads();                // (cut_s, whichever trip wrote it)
    if (tid == 0) {
        prefix[count] = carry;
        prefix[count + 1] = carry > kMaxCheckBlocks ? cut_s : carry;
    }
}

// block_status: null, or `count` pointers of which any may be null; container i's, when given, gets num_blocks words.
__global__ __launch_bounds__(64) void check_kernel(const StreamDesc* __restrict__ descs, uint32_t count, uint32_t* const* __restrict__ block_status,
                                                   uint32_t* __restrict__ results, const uint64_t* __restrict__ prefix, uint32_t* next_block)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t blocks = prefix[count + 1];

    for (;;) {
        const uint32_t p = draw_work(next_block, lane);
        if (p >= blocks) break;
        const uint32_t c = prefix_owner<true>(prefix, count, p);
        const StreamDesc d = descs[c];
        // validated by check_plan_kernel: block_size in [1, 65535], num_blocks = ceil(total_len / block_size)
        const uint8_t* stream = load_global_ptr(&descs[c].stream);
        const uint32_t b = p - (uint32_t)uld64(reinterpret_cast<const uint8_t*>(prefix + c));
        const uint64_t ostart = (uint64_t)b * d.block_size;
        const uint64_t oleft = d.total_len - ostart;
        const uint32_t out_len = oleft < d.block_size ? (uint32_t)oleft : d.block_size;
        const uint64_t at = uld64(reinterpret_cast<const uint8_t*>(load_global_ptr(&descs[c].block_offsets) + b));

        const uint32_t st = k2_check_block(stream, d.stream_len, at, out_len);

        if (lane == 0) {
            uint32_t* status = block_status ? load_global_ptr(&block_status[c]) : nullptr;
            if (status) status[b] = st;
            if (st != kBlockOk) {
                uint32_t* r = results + 4 * (uint64_t)c;
                atomicOr(r, kBlockInvalid);
                atomicAdd(r + 1, 1u);
                atomicMin(r + 2, b);
            }
        }
        // Keeps the wavefront together from one draw to the next (K2 and the range kernel end their trips the same way).
        // Without a convergent operation here the compiler threads the lanes that skip the `lane == 0` part straight into the
        // next trip's draw, apart from lane 0: they then read their own `drawn = 0` for ever.
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void raw_check_kernel(const RawItem* __restrict__ items, uint32_t count, uint64_t* __restrict__ out_len,
                                                       uint32_t* __restrict__ status, uint32_t* next_item)
{
    const uint32_t lane = threadIdx.x;

    for (;;) {
        const uint32_t i = draw_work(next_item, lane);
        if (i >= count) break;
        SNAPPY_RAW_CHECK_ITEM(items, i, out_len, status, lane)
        __syncthreads();            // (the wavefront stays together from one draw to the next: see check_kernel)
    }
}
#endif

}  // namespace snappy_hip
