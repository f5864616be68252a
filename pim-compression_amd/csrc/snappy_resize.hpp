// snappy_resize.hpp -- a block-framed container grown and shrunk in place: the first keep_len bytes of its plaintext kept, the
// bytes of a list of segments appended (snappy_hip_resize, include/snappy_hip.h).  Truncate = no segments, append = keep_len ==
// total_len, "rewrite from here on" = both.
//
// Blocks are independent in both directions and K1 is bit-identical to the reference per block, so
//     resize(container, keep_len, segments) == compress(plaintext[0:keep_len] + the segments' bytes), byte for byte,
// when every block wholly in front of keep_len ("kept", blocks 0 .. keep_len / block_size - 1) is copied and the others
// ("new", up to the new last block) are compressed: the first of them from the decoded head of the block keep_len cuts
// (keep_len % block_size bytes; nothing is decoded when keep_len lies on a block boundary) followed by segment bytes, the
// rest from segment bytes alone.  Blocks behind keep_len are never read.
// Two things differ from the update (snappy_update.hpp): the header's length changes with the new total_len, so a kept
// block's new offset is not its old one, and the last block's length changes, so K1 sizes its hash table anew (the
// compressor takes the block's own length, as for every short last block).
// Three kernels of its own, then the update's update_sizes_kernel and merge_stream_kernel, which take a kept block for a
// clean one (span[b], rank[b] == kNotDirty) and new block kept + k for dirty block k:
//   * resize_mark_kernel  (one thread per block of the NEW container): a kept block's chain link is checked (the rule of
//     verify_index_kernel) and its span kept; a new block gets its rank;
//   * resize_plan_kernel  (one workgroup): validates the shape, keep_len and the segments, scans the segments' lengths into
//     prefix[0 .. segment_count] and decides REJECTED;
//   * resize_recompress_kernel (persistent wavefronts, one counter): gathers new block kept + k into the wavefront's patch
//     slot -- K2's decoder for the cut block's head, wave_copy for the segments' pieces, found by binary search in the prefix --
//     and compresses the slot with K1's LDS-table form into compressed slot k.
// The LDS-table form only, as in the update and the raw compressor: a caller that appends gigabytes compresses the new data
// with snappy_hip_compress_blocks instead.
#pragma once
#include "snappy_update.hpp"    // the control line, kNotDirty, kPatchSlack, update_sizes_kernel, merge_stream_kernel

namespace snappy_hip {

struct SegmentDesc {           // must match snappy_hip_segment (include/snappy_hip.h)
    const uint8_t* src;
    uint64_t length;
};

// Scratch of one call, every part rounded up to 256 bytes: control line, prefix[segment_count + 1] (u64), span[new_blocks_all]
// (4 + size of a kept block), rank[new_blocks_all], new_bytes[compressed], `patch_slots` patch slots, `compressed` compressed
// slots.  new_blocks_all = blocks of the new container, compressed = those of them that are not kept.
// update_sizes_kernel and merge_stream_kernel are shared with the update, so this layout stays in step with UpdateLayout
// (snappy_update.hpp) where they look: span / rank per block, one u32 and one slot of slot_stride bytes per compressed block,
// patch slots of patch_slot_bytes = block_size + kPatchSlack rounded up to 256.
struct ResizeLayout {
    uint64_t prefix, span, rank, new_bytes, patch, cslots, total;
    uint32_t patch_slot_bytes, slot_stride;
};
__host__ __device__ inline ResizeLayout resize_layout(uint32_t block_size, uint32_t new_blocks_all, uint32_t compressed, uint32_t segment_count,
                                                      uint32_t patch_slots, uint32_t slot_stride)
{
    ResizeLayout l;
    l.patch_slot_bytes = (uint32_t)round256((uint64_t)block_size + kPatchSlack);
    l.slot_stride = slot_stride;
    l.prefix = 256;
    l.span = l.prefix + round256(((uint64_t)segment_count + 1u) * 8u);
    l.rank = l.span + round256((uint64_t)new_blocks_all * 4u);
    l.new_bytes = l.rank + round256((uint64_t)new_blocks_all * 4u);
    l.patch = l.new_bytes + round256((uint64_t)compressed * 4u);
    l.cslots = l.patch + (uint64_t)patch_slots * l.patch_slot_bytes;
    l.total = l.cslots + round256((uint64_t)compressed * slot_stride);
    return l;
}

__global__ __launch_bounds__(256) void resize_mark_kernel(const StreamDesc* __restrict__ desc, uint32_t total_len, uint32_t block_size,
                                                          uint32_t num_blocks, uint32_t keep_len, uint32_t new_num_blocks,
                                                          uint32_t* __restrict__ ctl, uint32_t* __restrict__ span, uint32_t* __restrict__ rank)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= new_num_blocks) return;
    const uint32_t kept = keep_len / block_size;
    if (b >= kept) {
        rank[b] = b - kept;
        return;
    }
    rank[b] = kNotDirty;
    const StreamDesc d = *desc;
    // (a descriptor of another shape and a keep_len beyond the container are REJECTED by resize_plan_kernel: no offset is read)
    if (d.total_len != total_len || d.block_size != block_size || d.num_blocks != num_blocks || keep_len > total_len) return;
    const uint8_t* stream = load_global_ptr(&desc->stream);
    const uint64_t* offsets = load_global_ptr(&desc->block_offsets);
    const uint64_t at = offsets[b];                          // (b < kept <= total_len / block_size <= num_blocks)
    const uint64_t next = b + 1 < num_blocks ? offsets[b + 1] : d.stream_len;
    uint32_t mine = 0;
    bool ok = at <= d.stream_len && d.stream_len - at >= 4;
    if (ok) {
        const uint64_t size = ld32(stream + at);
        ok = at + 4 + size == next && next <= d.stream_len && size < 0xfffffff0u;
        mine = (uint32_t)(4 + size);
    }
    if (!ok) {
        mine = 0;
        atomicOr(ctl + kCtlInvalid, 1u);
    }
    span[b] = mine;
}

__global__ __launch_bounds__(1024) void resize_plan_kernel(const StreamDesc* __restrict__ desc, uint32_t total_len, uint32_t block_size,
                                                           uint32_t num_blocks, uint32_t keep_len, uint32_t new_total_len,
                                                           uint32_t new_num_blocks, const SegmentDesc* __restrict__ segments,
                                                           uint32_t segment_count, uint32_t* __restrict__ segment_status,
                                                           uint32_t* __restrict__ ctl, uint64_t* __restrict__ prefix,
                                                           uint64_t* __restrict__ new_stream_len, uint32_t* __restrict__ result)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint32_t bad_s;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) bad_s = 0;
    __syncthreads();
    // the host's copies of the container's shape size the launches: they must be the descriptor's
    const StreamDesc d = *desc;
    bool bad = d.total_len != total_len || d.block_size != block_size || d.num_blocks != num_blocks || keep_len > total_len;
    // A length of 2^32 or more cannot be part of a sum that fits the format and is counted as 2^32 - 1: fewer than 2^32 such
    // terms and keep_len stay below 2^64, so the 64-bit sum below is the true one or the call is REJECTED already.
    uint64_t carry = 0;
    for (uint64_t base = 0; base < segment_count; base += 1024) {
        const uint64_t i = base + tid;
        uint64_t len = 0;
        if (i < segment_count) {
            const SegmentDesc s = segments[i];
            const uint32_t st = s.length && !s.src ? kRangeOutOfBounds : kBlockOk;
            segment_status[i] = st;
            bad |= st != kBlockOk || s.length > 0xffffffffull;
            len = s.length > 0xffffffffull ? 0xffffffffull : s.length;
        }
        uint64_t total;
        const uint64_t at = carry + workgroup_exclusive_scan(len, wave_sums, total);
        if (i < segment_count) prefix[i] = at;
        carry += total;
    }
    bad |= (uint64_t)keep_len + carry != new_total_len;
    if (bad) atomicOr(&bad_s, 1u);
    __syncthreads();
    if (tid == 0) {
        const bool rejected = bad_s != 0;
        const uint32_t kept = keep_len / block_size;
        prefix[segment_count] = carry;
        ctl[kCtlDirty] = rejected ? 0u : new_num_blocks - kept;   // (keep_len <= new_total_len here, so kept <= new_num_blocks)
        ctl[kCtlVerdict] = rejected ? kUpdateRejected : kBlockOk;
        if (rejected) {
            result[0] = kUpdateRejected;
            result[1] = 0;
            *new_stream_len = 0;
        }
    }
}

// kForm: the form of K1's parse the LDS-table kernel of the product runs at this block size (3 = stream, 2 = bulk); launched
// with that kernel's dynamic LDS, as recompress_dirty_kernel is
template <int kForm>
__global__ __launch_bounds__(64) void resize_recompress_kernel(const StreamDesc* __restrict__ desc, uint32_t total_len, uint32_t block_size,
                                                               uint32_t keep_len, uint32_t new_total_len,
                                                               const SegmentDesc* __restrict__ segments, uint32_t segment_count,
                                                               const uint64_t* __restrict__ prefix, uint32_t* __restrict__ ctl,
                                                               uint32_t* __restrict__ new_bytes, uint8_t* __restrict__ patch_slots,
                                                               uint32_t patch_slot_bytes, uint8_t* __restrict__ cslots, uint32_t slot_stride,
                                                               uint32_t* next_block)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage_mem[kK2StageBytes];   // one window's output (K2's stage)
    HIP_DYNAMIC_SHARED(uint8_t, lds_dyn)
    lds_bytes_t stage = (lds_bytes_t)stage_mem;
    const LdsTableWave k1(lds_dyn, block_size);
    const uint32_t lane = threadIdx.x;
    if (uni(ctl[kCtlVerdict]) != kBlockOk) return;
    const uint32_t count = uni(ctl[kCtlDirty]);
    const uint32_t kept = keep_len / block_size;
    uint8_t* slot = patch_slots + (uint64_t)blockIdx.x * patch_slot_bytes;

    for (;;) {
        const uint32_t k = draw_work(next_block, lane);
        if (k >= count) break;
        const uint32_t begin = (kept + k) * block_size;      // (validated: begin < new_total_len < 4 GiB)
        const uint32_t n = new_total_len - begin < block_size ? new_total_len - begin : block_size;
        const uint32_t head = k == 0 ? keep_len - begin : 0; // bytes of the block keep_len cuts that stay (keep_len % block_size)
        uint32_t st = kBlockOk;
        if (head) {
            // the cut block, decoded in full (its old length), as snappy_hip_decompress_blocks would
            const uint32_t old_n = total_len - begin < block_size ? total_len - begin : block_size;
            const uint8_t* stream = load_global_ptr(&desc->stream);
            const uint64_t* offsets = load_global_ptr(&desc->block_offsets);
            const uint64_t stream_len = uld64(reinterpret_cast<const uint8_t*>(&desc->stream_len));
            st = k2_decode_block(stream, stream_len, uld64(reinterpret_cast<const uint8_t*>(offsets + kept)), slot, old_n, stage);
            stores_landed();                                 // (the decode's)
        }
        if (st != kBlockOk) {
            if (lane == 0) {
                atomicOr(ctl + kCtlInvalid, 1u);
                new_bytes[k] = 0;
            }
        } else {
            // the block's bytes behind `head` are bytes [from, to) of the segments laid end to end
            const uint32_t from = begin + head - keep_len, to = begin + n - keep_len;
            for (uint32_t i = prefix_owner<true>(prefix, segment_count, from); i < segment_count; ++i) {
                const uint64_t s0 = uld64(reinterpret_cast<const uint8_t*>(prefix + i));
                if (s0 >= to) break;
                const uint64_t s1 = uld64(reinterpret_cast<const uint8_t*>(prefix + i + 1));
                const uint32_t lo = (uint32_t)(s0 > from ? s0 : from), hi = (uint32_t)(s1 < to ? s1 : to);
                if (hi > lo) wave_copy(slot + head + (lo - from), load_global_ptr(&segments[i].src) + (lo - s0), hi - lo, lane);
            }
            stores_landed();                                 // the gathered block is in memory before K1 reads it
            uint8_t* out = cslots + (uint64_t)k * slot_stride;
            LDS_TABLE_WAVE_COMPRESS(kForm, k1, slot, 0, n, n, out, lane, new_bytes + k);
        }
        __syncthreads();
    }
}

}  // namespace snappy_hip
