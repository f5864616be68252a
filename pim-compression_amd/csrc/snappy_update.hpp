// snappy_update.hpp -- byte ranges of a block-framed container overwritten, recompressing only the blocks they touch
// (snappy_hip_update_ranges, include/snappy_hip.h).
//
// Blocks are independent in both directions and K1 is bit-identical to the reference per block, so
//     update(container, writes) == compress(plaintext with the writes applied), byte for byte,
// when only the touched ("dirty") blocks are decoded, patched and recompressed and every other block's bytes are copied.
// Five kernels, all reading their verdicts from the scratch (the host is never asked):
//   * update_mark_kernel   (one thread per block): binary search of the sorted writes for "touched"; a clean block's chain
//     link is checked (the rule of verify_index_kernel) and its span kept;
//   * update_plan_kernel   (one workgroup): validates the writes (bounds, order against the predecessor), scans the dirty
//     flags into rank[b] / dirty[k] and decides REJECTED;
//   * recompress_dirty_kernel (persistent wavefronts, one counter): dirty block dirty[k] is decoded with K2's own decoder
//     into the wavefront's patch slot (not when the writes cover it completely), the writes' pieces are laid over it and the
//     slot is compressed with K1's LDS-table form into compressed slot k;
//   * update_sizes_kernel  (one workgroup): new size per block, capacity check, then the scan into the new offsets and the
//     header;
//   * merge_stream_kernel  (one workgroup per block): copies the block from the old stream or from its compressed slot.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_kernels.hpp"   // StreamDesc, k2_decode_block, LdsTableWave

namespace snappy_hip {

constexpr uint32_t kWriteUnordered = 3;      // SNAPPY_HIP_WRITE_UNORDERED
constexpr uint32_t kUpdateRejected = 4;      // SNAPPY_HIP_UPDATE_REJECTED
constexpr uint32_t kNotDirty = 0xffffffffu;  // rank[b] of a clean block
constexpr uint32_t kPatchSlack = 64;         // bytes behind a patch slot's block (K1's loads are clamped to the block; spare anyway)

struct WriteDesc {             // must match snappy_hip_write (include/snappy_hip.h)
    uint64_t offset;
    uint64_t length;
    const uint8_t* src;
    uint64_t pad;
};

// words of the control line at the start of the scratch (zeroed by the call)
enum : uint32_t { kCtlVerdict = 0, kCtlDirty = 1, kCtlInvalid = 2, kCtlGo = 3 };

// Scratch of one call, every part rounded up to 256 bytes: control line, span[num_blocks] (4 + size of a clean block),
// rank[num_blocks], dirty[max_dirty], dirty_bytes[max_dirty], `patch_slots` patch slots, max_dirty compressed slots.
struct UpdateLayout {
    uint64_t span, rank, dirty, dirty_bytes, patch, cslots, total;
    uint32_t patch_slot_bytes, slot_stride;
};
__host__ __device__ inline UpdateLayout update_layout(uint32_t block_size, uint32_t num_blocks, uint32_t max_dirty, uint32_t patch_slots,
                                                      uint32_t slot_stride)
{
    UpdateLayout l;
    l.patch_slot_bytes = (uint32_t)round256((uint64_t)block_size + kPatchSlack);
    l.slot_stride = slot_stride;
    l.span = 256;
    l.rank = l.span + round256((uint64_t)num_blocks * 4u);
    l.dirty = l.rank + round256((uint64_t)num_blocks * 4u);
    l.dirty_bytes = l.dirty + round256((uint64_t)max_dirty * 4u);
    l.patch = l.dirty_bytes + round256((uint64_t)max_dirty * 4u);
    l.cslots = l.patch + (uint64_t)patch_slots * l.patch_slot_bytes;
    l.total = l.cslots + round256((uint64_t)max_dirty * slot_stride);
    return l;
}

// end of a write, saturated (an overflowing write is out of bounds itself and puts every later one out of order)
__device__ __forceinline__ uint64_t write_end(const WriteDesc& w) { return w.offset + w.length < w.offset ? ~0ull : w.offset + w.length; }

// first write whose end lies behind `pos` (write_count if none); the ends of sorted, disjoint writes do not decrease
__device__ __forceinline__ uint32_t first_write_behind(const WriteDesc* __restrict__ writes, uint32_t write_count, uint64_t pos)
{
    uint32_t lo = 0, hi = write_count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (write_end(writes[mid]) > pos) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void update_mark_kernel(const StreamDesc* __restrict__ desc, uint32_t total_len, uint32_t block_size,
                                                          uint32_t num_blocks, const WriteDesc* __restrict__ writes, uint32_t write_count,
                                                          uint32_t* __restrict__ ctl, uint32_t* __restrict__ span)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= num_blocks) return;
    const StreamDesc d = *desc;
    // (a descriptor of another shape is REJECTED by update_plan_kernel: its offsets are not read)
    if (d.total_len != total_len || d.block_size != block_size || d.num_blocks != num_blocks) return;
    const uint64_t begin = (uint64_t)b * block_size;
    const uint64_t end = begin + block_size < total_len ? begin + block_size : total_len;
    bool touched = false;
    for (uint32_t i = first_write_behind(writes, write_count, begin); i < write_count && writes[i].offset < end; ++i)
        if (writes[i].length) {       // (writes of no bytes dirty nothing)
            touched = true;
            break;
        }
    uint32_t mine = kNotDirty;
    if (!touched) {
        const uint8_t* stream = load_global_ptr(&desc->stream);
        const uint64_t* offsets = load_global_ptr(&desc->block_offsets);
        const uint64_t at = offsets[b];
        const uint64_t next = b + 1 < num_blocks ? offsets[b + 1] : d.stream_len;
        bool ok = at <= d.stream_len && d.stream_len - at >= 4;
        if (ok) {
            const uint64_t size = ld32(stream + at);
            ok = at + 4 + size == next && next <= d.stream_len && size < 0xfffffff0u;   // (a span must not read as kNotDirty)
            mine = (uint32_t)(4 + size);
        }
        if (!ok) {
            mine = 0;
            atomicOr(ctl + kCtlInvalid, 1u);
        }
    }
    span[b] = mine;                  // kNotDirty here = "touched": a span is at most 4 + 2^32 - 1 only when the link is broken
}

__global__ __launch_bounds__(1024) void update_plan_kernel(const StreamDesc* __restrict__ desc, uint32_t total_len, uint32_t block_size,
                                                           uint32_t num_blocks, const WriteDesc* __restrict__ writes, uint32_t write_count,
                                                           uint32_t* __restrict__ write_status, uint32_t max_dirty,
                                                           uint32_t* __restrict__ ctl, const uint32_t* __restrict__ span,
                                                           uint32_t* __restrict__ rank, uint32_t* __restrict__ dirty,
                                                           uint64_t* __restrict__ new_stream_len, uint32_t* __restrict__ result)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint32_t bad_s;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) bad_s = 0;
    __syncthreads();
    // the host's copies of the container's shape size the launches: they must be the descriptor's
    const StreamDesc d = *desc;
    bool bad = d.total_len != total_len || d.block_size != block_size || d.num_blocks != num_blocks;
    for (uint32_t i = tid; i < write_count; i += 1024) {
        const WriteDesc w = writes[i];
        uint32_t st = kBlockOk;
        if (i > 0 && w.offset < write_end(writes[i - 1])) st = kWriteUnordered;
        if (w.offset + w.length < w.offset || w.offset + w.length > total_len || (w.length && !w.src)) st = kRangeOutOfBounds;
        write_status[i] = st;
        bad |= st != kBlockOk;
    }
    if (bad) atomicOr(&bad_s, 1u);
    __syncthreads();
    bad = bad_s != 0;

    uint64_t carry = 0;
    if (!bad)
        for (uint32_t base = 0; base < num_blocks; base += 1024) {
            const uint32_t b = base + tid;
            const bool is_dirty = b < num_blocks && span[b] == kNotDirty;
            uint64_t total;
            const uint64_t k = carry + workgroup_exclusive_scan(is_dirty ? 1u : 0u, wave_sums, total);
            if (b < num_blocks) rank[b] = is_dirty ? (uint32_t)k : kNotDirty;
            if (is_dirty && k < max_dirty) dirty[k] = b;
            carry += total;
        }
    if (tid == 0) {
        const bool rejected = bad || carry > max_dirty;
        ctl[kCtlDirty] = rejected ? 0u : (uint32_t)carry;
        ctl[kCtlVerdict] = rejected ? kUpdateRejected : kBlockOk;
        if (rejected) {
            result[0] = kUpdateRejected;
            result[1] = bad ? 0u : (uint32_t)carry;
            *new_stream_len = 0;
        }
    }
}

// kForm: the form of K1's parse the LDS-table kernel of the product runs at this block size (3 = stream, 2 = bulk); launched
// with that kernel's dynamic LDS (lds_table_stream_lds_bytes / lds_table_kernel_lds_bytes)
template <int kForm>
__global__ __launch_bounds__(64) void recompress_dirty_kernel(const StreamDesc* __restrict__ desc, uint32_t total_len, uint32_t block_size,
                                                              const WriteDesc* __restrict__ writes, uint32_t write_count,
                                                              uint32_t* __restrict__ ctl, const uint32_t* __restrict__ dirty,
                                                              uint32_t* __restrict__ dirty_bytes, uint8_t* __restrict__ patch_slots,
                                                              uint32_t patch_slot_bytes, uint8_t* __restrict__ cslots, uint32_t slot_stride,
                                                              uint32_t* next_dirty)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage_mem[kK2StageBytes];   // one window's output (K2's stage)
    HIP_DYNAMIC_SHARED(uint8_t, lds_dyn)
    lds_bytes_t stage = (lds_bytes_t)stage_mem;
    const LdsTableWave k1(lds_dyn, block_size);
    const uint32_t lane = threadIdx.x;
    if (uni(ctl[kCtlVerdict]) != kBlockOk) return;
    const uint32_t count = uni(ctl[kCtlDirty]);
    uint8_t* slot = patch_slots + (uint64_t)blockIdx.x * patch_slot_bytes;
    const uint8_t* stream = load_global_ptr(&desc->stream);
    const uint64_t* offsets = load_global_ptr(&desc->block_offsets);
    const uint64_t stream_len = uld64(reinterpret_cast<const uint8_t*>(&desc->stream_len));

    for (;;) {
        const uint32_t k = draw_work(next_dirty, lane);
        if (k >= count) break;
        const uint32_t b = uni(dirty[k]);
        const uint32_t begin = b * block_size;               // (validated: total_len < 4 GiB)
        const uint32_t n = total_len - begin < block_size ? total_len - begin : block_size;
        const uint32_t end = begin + n;
        const uint32_t first = first_write_behind(writes, write_count, begin);
        // bytes of the block the writes bring (they are disjoint): all of them = the old block cannot matter
        uint32_t covered = 0;
        for (uint32_t i = first; i < write_count; ++i) {
            const uint64_t wo = uld64(reinterpret_cast<const uint8_t*>(&writes[i].offset));
            if (wo >= end) break;
            const uint64_t we = wo + uld64(reinterpret_cast<const uint8_t*>(&writes[i].length));
            covered += (uint32_t)((we < end ? we : end) - (wo > begin ? wo : begin));
        }
        uint32_t st = kBlockOk;
        if (covered < n) {
            st = k2_decode_block(stream, stream_len, uld64(reinterpret_cast<const uint8_t*>(offsets + b)), slot, n, stage);
            stores_landed();                                 // (the decode's)
        }
        if (st != kBlockOk) {
            if (lane == 0) {
                atomicOr(ctl + kCtlInvalid, 1u);
                dirty_bytes[k] = 0;
            }
        } else {
            for (uint32_t i = first; i < write_count; ++i) {
                const uint64_t wo = uld64(reinterpret_cast<const uint8_t*>(&writes[i].offset));
                if (wo >= end) break;
                const uint64_t we = wo + uld64(reinterpret_cast<const uint8_t*>(&writes[i].length));
                const uint32_t from = (uint32_t)(wo > begin ? wo : begin), to = (uint32_t)(we < end ? we : end);
                if (to > from) wave_copy(slot + (from - begin), load_global_ptr(&writes[i].src) + (from - wo), to - from, lane);
            }
            stores_landed();                                 // the patched block is in memory before K1 reads it
            uint8_t* out = cslots + (uint64_t)k * slot_stride;
            LDS_TABLE_WAVE_COMPRESS(kForm, k1, slot, 0, n, n, out, lane, dirty_bytes + k);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void update_sizes_kernel(uint32_t total_len, uint32_t block_size, uint32_t num_blocks,
                                                            uint32_t* __restrict__ ctl, const uint32_t* __restrict__ span,
                                                            const uint32_t* __restrict__ rank, const uint32_t* __restrict__ dirty_bytes,
                                                            uint8_t* __restrict__ new_stream, uint64_t capacity,
                                                            uint64_t* __restrict__ new_offsets, uint64_t* __restrict__ new_stream_len,
                                                            uint32_t* __restrict__ result)
{
    __shared__ uint64_t wave_sums[16];
    const uint32_t tid = threadIdx.x;
    if (ctl[kCtlVerdict] != kBlockOk) return;                // REJECTED by the plan: everything is said
    if (ctl[kCtlInvalid]) {
        if (tid == 0) {
            result[0] = kBlockInvalid;
            result[1] = ctl[kCtlDirty];
            *new_stream_len = 0;
        }
        return;
    }
    const uint32_t hdr_len = varint32_len(total_len) + varint32_len(block_size);
    auto size_of = [&](uint32_t b) -> uint64_t { return rank[b] == kNotDirty ? span[b] : dirty_bytes[rank[b]]; };
    // first the length alone: a stream that does not fit leaves no byte behind
    uint64_t mine = 0;
    for (uint32_t b = tid; b < num_blocks; b += 1024) mine += size_of(b);
    uint64_t new_len;
    (void)workgroup_exclusive_scan(mine, wave_sums, new_len);
    new_len += hdr_len;
    if (new_len > capacity) {
        if (tid == 0) {
            result[0] = kUpdateRejected;
            result[1] = ctl[kCtlDirty];
            *new_stream_len = 0;
        }
        return;
    }
    uint64_t carry = hdr_len;
    for (uint32_t base = 0; base < num_blocks; base += 1024) {
        const uint32_t b = base + tid;
        uint64_t total;
        const uint64_t at = carry + workgroup_exclusive_scan(b < num_blocks ? size_of(b) : 0u, wave_sums, total);
        if (b < num_blocks) new_offsets[b] = at;
        carry += total;
    }
    if (tid == 0) {
        put_varint32(new_stream + put_varint32(new_stream, total_len), block_size);
        new_offsets[num_blocks] = carry;
        *new_stream_len = carry;
        result[0] = kBlockOk;
        result[1] = ctl[kCtlDirty];
        ctl[kCtlGo] = 1;
    }
}

// One 256-thread workgroup per block: new_offsets[b + 1] - new_offsets[b] bytes from the old stream (a clean block) or from
// the block's compressed slot to new_stream + new_offsets[b]; both ends at any alignment (workgroup_copy).
__global__ __launch_bounds__(256) void merge_stream_kernel(const StreamDesc* __restrict__ desc, uint32_t num_blocks,
                                                           const uint32_t* __restrict__ ctl, const uint32_t* __restrict__ rank,
                                                           const uint8_t* __restrict__ cslots, uint32_t slot_stride,
                                                           const uint64_t* __restrict__ new_offsets, uint8_t* __restrict__ new_stream)
{
    if (ctl[kCtlGo] != 1u) return;
    const uint8_t* old_stream = load_global_ptr(&desc->stream);
    const uint64_t* old_offsets = load_global_ptr(&desc->block_offsets);
    for (uint32_t b = blockIdx.x; b < num_blocks; b += gridDim.x) {
        const uint32_t k = rank[b];
        const uint8_t* src = k == kNotDirty ? old_stream + old_offsets[b] : cslots + (uint64_t)k * slot_stride;
        const uint64_t at = new_offsets[b];
        workgroup_copy(new_stream + at, src, (uint32_t)(new_offsets[b + 1] - at));
    }
}

}  // namespace snappy_hip
