// snappy_raw.hpp -- batches of ORIGINAL ("raw") Snappy streams, described on the device (snappy_hip_raw_decompress_batch,
// snappy_hip_raw_compress_batch, include/snappy_hip.h).
//
// A raw stream is varint32(uncompressed length) + ONE element stream whose back-references may reach back as far as the
// stream is long: what Parquet / ORC pages, Arrow IPC buffers and `snzip -t raw` hold.  An item is (src, src_len, dst,
// dst_capacity), read from device memory.
//   * decode: raw_decompress_kernel (persistent wavefronts, one counter, as decompress_ranges_kernel): a wavefront draws an
//     item, reads its header and decodes the whole stream with K2's own decoder in its raw form (k2_decode_block<true>:
//     literals of any length, 64-bit bounds against the stream, wide run-on copies).  Element boundaries of a raw stream cannot
//     be found without parsing it, so ONE STREAM IS ONE WAVEFRONT'S WORK here; the device is full only with thousands of items.
//     (snappy_raw_split.hpp decodes one LARGE stream with many wavefronts, and shares this kernel's trip.)
//   * compress: a FRAGMENT is block_size bytes of an item, compressed as one K1 block (own hash table, no reference across
//     fragments -- what Google's compressor does with its 64 KiB fragments, so any decoder accepts the result).  The work unit
//     is the pair (item, fragment), found from the exclusive prefix of the items' fragment counts by binary search.  Four
//     kernels, the update's pipeline: raw_plan_kernel (one workgroup: validates the items, counts and prefixes the fragments),
//     raw_compress_fragments_kernel (persistent wavefronts, K1's LDS-table form, fragment f into slot f of the scratch),
//     raw_sizes_kernel (a wavefront per item: size, capacity verdict, header, each fragment's place in dst) and
//     raw_gather_kernel (a workgroup per fragment: the payload without its u32 size word, any alignment on both sides).
//     Item i's output is byte for byte tools/to_raw_snappy.py convert() of the framed stream of the same plaintext.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_kernels.hpp"   // k2_decode_block, LdsTableWave

namespace snappy_hip {

constexpr uint32_t kRawDstTooSmall = 5;      // SNAPPY_HIP_RAW_DST_TOO_SMALL
constexpr uint32_t kRawTooLarge = 6;         // SNAPPY_HIP_RAW_TOO_LARGE
// The longest stream and the longest output the decoder takes (SNAPPY_HIP_RAW_MAX_LEN).  K2's cursors are 32 bits wide.  With
// csz, out_len <= M: a compressed cursor never exceeds csz + 200 (window base + 128 + 72 in issue()); an element predecode
// accepted ends inside the stream (64-bit test), so a literal is at most M long; one window's output `total` is at most that
// literal + 1408 bytes of copies, and op <= out_len when `op + total > out_len` is evaluated: op + total <= 2 M + 1408, which
// must stay below 2^32.  M = 2^31 - 4096 is the largest page multiple that does.
constexpr uint64_t kRawMaxLen = 0x7ffff000ull;

struct RawItem {               // must match snappy_hip_raw_item (include/snappy_hip.h)
    const uint8_t* src;
    uint64_t src_len;
    uint8_t* dst;
    uint64_t dst_capacity;
};

// The descriptor and the header of item i and the item's verdict, by the rules every raw decoder shares: a null src or a
// malformed header is INVALID with a length of 0, a stream or a length above kRawMaxLen is TOO_LARGE, a length above the
// capacity (a null dst counts as 0) DST_TOO_SMALL, a length of 0 is OK iff nothing follows the header; for every other item
// the verdict is `elements`, an expression over src, src_len, hdr, dst and length: its elements src[hdr, src_len) are to be
// decoded into dst[0, length).  Declares those five, capacity and `uint32_t st` in the caller's scope.  uld / ubyte: uld64 /
// uni when the whole wavefront reads ONE item (i wave-uniform, everything lands in scalar registers), ld64 / a plain cast
// when every thread reads an item of its own.  A macro, so that raw_decompress_kernel's text -- and with it its generated
// code, which tools/kernel_asm_diff.py holds to what it was measured with -- stays what it was while raw_split_plan_kernel and
// raw_split_serial_kernel (snappy_raw_split.hpp) read the same rules.
#define SNAPPY_RAW_ITEM_VERDICT(items, i, uld, ubyte, elements)                                                                \
    const uint8_t* src = load_global_ptr(&items[i].src);                                                                       \
    uint8_t* dst = load_global_ptr(&items[i].dst);                                                                             \
    const uint64_t src_len = uld(reinterpret_cast<const uint8_t*>(&items[i].src_len));                                         \
    const uint64_t capacity = dst ? uld(reinterpret_cast<const uint8_t*>(&items[i].dst_capacity)) : 0;                         \
    /* the header: a varint32 as Google's decoder reads it -- at most 5 bytes, the fifth below 16, inside the stream */         \
    uint32_t length = 0, hdr = 0;                                                                                              \
    if (src)                                                                                                                   \
        for (uint32_t k = 0; k < 5 && k < src_len; ++k) {                                                                      \
            const uint32_t c = ubyte((uint32_t)src[k]);                                                                        \
            if (k == 4 && c >= 16u) break;                                                                                     \
            length |= (c & 0x7fu) << (7u * k);                                                                                 \
            if (c < 0x80u) {                                                                                                   \
                hdr = k + 1;                                                                                                   \
                break;                                                                                                         \
            }                                                                                                                  \
        }                                                                                                                      \
    uint32_t st;                                                                                                               \
    if (hdr == 0) {                                                                                                            \
        st = kBlockInvalid;                                                                                                    \
        length = 0;                                                                                                            \
    } else if (src_len > kRawMaxLen || length > kRawMaxLen) {                                                                  \
        st = kRawTooLarge;                                                                                                     \
    } else if (length > capacity) {                                                                                            \
        st = kRawDstTooSmall;                                                                                                  \
    } else if (length == 0) {                                                                                                  \
        st = src_len == hdr ? kBlockOk : kBlockInvalid; /* nothing may follow the header */                                    \
    } else {                                                                                                                   \
        st = (elements);                                                                                                       \
    }

// One item decoded by ONE wavefront, verdict and length stored: a trip of raw_decompress_kernel and of the split call's serial
// step.  i is wave-uniform; every lane of the wavefront runs it.
#define SNAPPY_RAW_DECODE_ITEM(items, i, out_len, status, stage, lane)                                                         \
    SNAPPY_RAW_ITEM_VERDICT(items, i, uld64, uni, k2_decode_block<true>(src, src_len, hdr, dst, length, stage))                \
    if (lane == 0) {                                                                                                           \
        status[i] = st;                                                                                                        \
        out_len[i] = length;                                                                                                   \
    }

#ifndef SNAPPY_HIP_NO_KERNELS
__global__ __launch_bounds__(64) void raw_decompress_kernel(const RawItem* __restrict__ items, uint32_t count, uint64_t* __restrict__ out_len,
                                                            uint32_t* __restrict__ status, uint32_t* next_item)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage_mem[kK2StageBytes];   // one window's output (K2's stage)
    lds_bytes_t stage = (lds_bytes_t)stage_mem;
    const uint32_t lane = threadIdx.x;

    for (;;) {
        const uint32_t i = draw_work(next_item, lane);
        if (i >= count) break;
        SNAPPY_RAW_DECODE_ITEM(items, i, out_len, status, stage, lane)
        __syncthreads();
    }
}
#endif

// ---- compress ----
// words of the control line at the start of the scratch
enum : uint32_t { kRawCtlFragments = 0 };    // fragments to compress: those of the items in front of the first one beyond max_fragments

// Scratch of one call, every part rounded up to 256 bytes: control line, prefix[count + 1] (u64: first fragment of item i;
// [count] = all fragments), frag_bytes[max_fragments] (u32: 4 + payload, as K1 leaves it), place[max_fragments] (u64: the
// payload's offset in its item's dst), max_fragments compressed slots.
struct RawLayout {
    uint64_t prefix, frag_bytes, place, slots, total;
};
__host__ __device__ inline RawLayout raw_layout(uint32_t count, uint32_t max_fragments, uint32_t slot_stride)
{
    RawLayout l;
    l.prefix = 256;
    l.frag_bytes = l.prefix + round256(((uint64_t)count + 1u) * 8u);
    l.place = l.frag_bytes + round256((uint64_t)max_fragments * 4u);
    l.slots = l.place + round256((uint64_t)max_fragments * 8u);
    l.total = l.slots + round256((uint64_t)max_fragments * slot_stride);
    return l;
}

#ifndef SNAPPY_HIP_NO_KERNELS
__global__ __launch_bounds__(1024) void raw_plan_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t block_size,
                                                        uint32_t max_fragments, uint64_t* __restrict__ out_len, uint32_t* __restrict__ status,
                                                        uint32_t* __restrict__ result, uint32_t* __restrict__ ctl, uint64_t* __restrict__ prefix)
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
            else mine = (q.src_len + block_size - 1) / block_size;
        }
        uint64_t total;
        const uint64_t first = carry + workgroup_exclusive_scan(mine, wave_sums, total);
        if (i < count) {
            prefix[i] = first;
            // past max_fragments: the item that straddles it (exactly one when there are more fragments) marks the cut
            const bool beyond = mine && first + mine > max_fragments;
            if (beyond && first <= max_fragments) cut_s = first;
            status[i] = beyond ? kRawTooLarge : st;
            out_len[i] = 0;
        }
        carry += total;
    }
    __syncthreads();                // (cut_s, whichever trip wrote it)
    if (tid == 0) {
        prefix[count] = carry;
        ctl[kRawCtlFragments] = (uint32_t)(carry > max_fragments ? cut_s : carry);
        result[0] = carry > 0xffffffffull ? 0xffffffffu : (uint32_t)carry;
        result[1] = 0;
    }
}
#endif

// kForm: the form of K1's parse the LDS-table kernel of the product runs at this block size (3 = stream, 2 = bulk); launched
// with that kernel's dynamic LDS (lds_table_stream_lds_bytes / lds_table_kernel_lds_bytes)
template <int kForm>
__global__ __launch_bounds__(64) void raw_compress_fragments_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t block_size,
                                                                    const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ prefix,
                                                                    uint32_t* __restrict__ frag_bytes, uint8_t* __restrict__ slots,
                                                                    uint32_t slot_stride, uint32_t* next_fragment)
{
    HIP_DYNAMIC_SHARED(uint8_t, lds_dyn)
    const LdsTableWave k1(lds_dyn, block_size);
    const uint32_t lane = threadIdx.x;
    const uint32_t fragments = uni(ctl[kRawCtlFragments]);

    for (;;) {
        const uint32_t f = draw_work(next_fragment, lane);
        if (f >= fragments) break;
        const uint32_t i = prefix_owner<false>(prefix, count, f);
        const uint8_t* src = load_global_ptr(&items[i].src);
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));   // (validated: < 4 GiB)
        const uint64_t start = (f - uld64(reinterpret_cast<const uint8_t*>(prefix + i))) * block_size;
        const uint64_t left = src_len - start;
        const uint32_t n = left < block_size ? (uint32_t)left : block_size;
        uint8_t* out = slots + (uint64_t)f * slot_stride;
        LDS_TABLE_WAVE_COMPRESS(kForm, k1, src, start, src_len, n, out, lane, frag_bytes + f);
        __syncthreads();
    }
}

// One wavefront per item the plan left OK: the sizes of its fragments' payloads are scanned into their places behind the
// header; an item that does not fit its dst is told the size it needs and keeps every byte of dst.
#ifndef SNAPPY_HIP_NO_KERNELS
__global__ __launch_bounds__(64) void raw_sizes_kernel(const RawItem* __restrict__ items, uint32_t count, const uint64_t* __restrict__ prefix,
                                                       const uint32_t* __restrict__ frag_bytes, uint64_t* __restrict__ place,
                                                       uint64_t* __restrict__ out_len, uint32_t* __restrict__ status, uint32_t* __restrict__ result)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        if (uni(status[i]) != kBlockOk) continue;
        const uint64_t first = uld64(reinterpret_cast<const uint8_t*>(prefix + i)), end = uld64(reinterpret_cast<const uint8_t*>(prefix + i + 1));
        const uint32_t src_len = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
        uint64_t at = varint32_len(src_len);
        for (uint64_t base = first; base < end; base += kWave) {
            const uint64_t f = base + lane;
            const uint32_t mine = f < end ? frag_bytes[f] - 4u : 0u;
            const uint32_t x = wave_inclusive_scan(mine, lane);
            if (f < end) place[f] = at + (x - mine);
            at += (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
        }
        uint8_t* dst = load_global_ptr(&items[i].dst);
        const uint64_t capacity = dst ? uld64(reinterpret_cast<const uint8_t*>(&items[i].dst_capacity)) : 0;
        if (lane == 0) {
            out_len[i] = at;
            if (at > capacity) {
                status[i] = kRawDstTooSmall;
            } else {
                put_varint32(dst, src_len);
                atomicAdd(result + 1, 1u);
            }
        }
    }
}

// One 256-thread workgroup per fragment: frag_bytes[f] - 4 bytes from behind the size word of slot f to the fragment's place
// in its item's dst; both ends at any alignment (workgroup_copy, as merge_stream_kernel).
__global__ __launch_bounds__(256) void raw_gather_kernel(const RawItem* __restrict__ items, uint32_t count, const uint32_t* __restrict__ ctl,
                                                         const uint64_t* __restrict__ prefix, const uint32_t* __restrict__ frag_bytes,
                                                         const uint64_t* __restrict__ place, const uint8_t* __restrict__ slots,
                                                         uint32_t slot_stride, const uint32_t* __restrict__ status)
{
    const uint32_t fragments = ctl[kRawCtlFragments];
    for (uint32_t f = blockIdx.x; f < fragments; f += gridDim.x) {
        const uint32_t i = prefix_owner<false>(prefix, count, f);
        if (status[i] != kBlockOk) continue;
        const uint8_t* src = slots + (uint64_t)f * slot_stride + 4;
        uint8_t* dst = load_global_ptr(&items[i].dst) + place[f];
        workgroup_copy(dst, src, frag_bytes[f] - 4u);
    }
}
#endif

}  // namespace snappy_hip
