// snappy_hip_sz_split.hip -- the fourth source of libsnappy_hip.so: the chunk chain of one large .sz stream walked by many
// wavefronts (snappy_sz_split.hpp; snappy_hip_sz_decompress_split_batch, include/snappy_hip.h).
//
// As snappy_hip_sz.hip: a new feature's kernels live in a source of their own.  This one takes the __device__ pieces of the other
// headers without their kernels (SNAPPY_HIP_NO_KERNELS, and SNAPPY_SZ_NO_KERNELS for snappy_sz.hpp), launches only kernels it
// defines itself, and enqueues the plan, the decode and the finish of snappy_hip_sz.hip through host_shared.hpp.
#define SNAPPY_HIP_NO_KERNELS
#define SNAPPY_SZ_NO_KERNELS
#undef SNAPPY_PROF          // (the probe builds' counters are snappy_hip.hip's own)
#undef SNAPPY_PAIR_PROBE
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/snappy_hip.h"
#include "host_shared.hpp"
#include "snappy_sz_split.hpp"

using namespace snappy_hip_host;

static bool sz_split_params(uint32_t& segment_bytes)
{
    if (segment_bytes == 0) segment_bytes = snappy_hip::kSzSplitDefaultSegment;
    return segment_bytes >= snappy_hip::kSzSplitMinSegment && segment_bytes % 64u == 0;
}

namespace snappy_hip_host {

bool sz_split_segment_ok(uint32_t& segment_bytes) { return sz_split_params(segment_bytes); }

uint64_t sz_split_scratch_total(uint32_t count, uint32_t max_chunks, uint64_t max_segments)
{
    return snappy_hip::sz_split_layout(count, max_chunks, max_segments).total;
}

int sz_split_enqueue_walk(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t max_chunks, uint32_t segment_bytes,
                          uint64_t max_segments, uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch)
{
    using namespace snappy_hip;
    const SzSplitLayout l = sz_split_layout(count, max_chunks, max_segments);
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(scratch);
    uint64_t* prefix = reinterpret_cast<uint64_t*>(scratch + l.d.prefix);
    SzChunk* chunks = reinterpret_cast<SzChunk*>(scratch + l.d.chunks);
    uint64_t* seg_prefix = reinterpret_cast<uint64_t*>(scratch + l.seg_prefix);
    uint32_t* item_flags = reinterpret_cast<uint32_t*>(scratch + l.flags);
    SzSeg* segs = reinterpret_cast<SzSeg*>(scratch + l.segs);
    const auto* items = reinterpret_cast<const RawItem*>(d_items);
    hipLaunchKernelGGL(sz_split_plan_kernel, dim3(1), dim3(1024), 0, st, items, count, segment_bytes, max_segments, d_out_len, d_status, d_result, ctl,
                       prefix, seg_prefix, item_flags);
    HIP_TRY(hipGetLastError());
    // a wavefront per segment: the walkers wait on one miss per chunk, so as many of them as there are segments, up to four rounds
    // of the persistent kernels' grid
    const uint32_t seg_grid = (uint32_t)std::min<uint64_t>(4ull * range_grid_cap(), max_segments);
    const uint32_t item_grid = std::min(std::max(count, 1u), 4096u);
    if (count) {
        if (seg_grid) {                 // (else no item can be spread: step 4 walks them all)
            hipLaunchKernelGGL(sz_split_anchor_kernel, dim3(seg_grid), dim3(64), 0, st, items, count, segment_bytes, ctl, seg_prefix, segs);
            hipLaunchKernelGGL(sz_split_walk_kernel, dim3(seg_grid), dim3(64), 0, st, items, count, segment_bytes, ctl, seg_prefix, segs);
        }
        hipLaunchKernelGGL(sz_split_join_kernel, dim3(item_grid), dim3(64), 0, st, items, count, max_chunks, d_out_len, d_status, prefix, chunks,
                           seg_prefix, item_flags, segs, d_result);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = sz_enqueue_plan(st, count, max_chunks, d_status, d_result, d_scratch)) return rc;
    if (count == 0) return 0;
    if (max_chunks) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)seg_grid + item_grid, 65536u);
        hipLaunchKernelGGL(sz_split_record_kernel, dim3(grid), dim3(64), 0, st, items, count, segment_bytes, ctl, d_status, prefix, chunks, seg_prefix,
                           item_flags, segs);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace snappy_hip_host

extern "C" {

uint64_t snappy_hip_sz_decompress_split_scratch_bytes(uint32_t count, uint32_t max_chunks, uint32_t segment_bytes, uint64_t max_segments)
{
    if (!sz_split_params(segment_bytes)) return 0;
    return snappy_hip::sz_split_layout(count, max_chunks, max_segments).total;
}

int snappy_hip_sz_decompress_split_batch(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t max_chunks, uint32_t segment_bytes,
                                         uint64_t max_segments, uint32_t flags, uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_bad_chunk,
                                         uint32_t* d_result, void* d_scratch, uint64_t scratch_bytes, void* stream)
{
    using namespace snappy_hip;
    static_assert(sizeof(snappy_hip_raw_item) == sizeof(RawItem), "snappy_hip_raw_item layout");
    if (!sz_split_params(segment_bytes)) return fail(SNAPPY_HIP_ERR_ARG, "segment_bytes must be 0 or a multiple of 64 of at least 256");
    if (flags & ~SNAPPY_HIP_SZ_NO_VERIFY) return fail(SNAPPY_HIP_ERR_ARG, "unknown flag (SNAPPY_HIP_SZ_NO_VERIFY is the only one)");
    if (!d_result || (count && (!d_items || !d_out_len || !d_status || !d_bad_chunk))) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    max_segments = std::min(max_segments, kSzSplitMaxSegments);
    const SzSplitLayout l = sz_split_layout(count, max_chunks, max_segments);
    if (scratch_bytes < l.total) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_sz_decompress_split_scratch_bytes)");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sz_split_enqueue_walk(st, d_items, count, max_chunks, segment_bytes, max_segments, d_out_len, d_status, d_result, d_scratch)) return rc;
    if (count == 0) return SNAPPY_HIP_OK;
    return sz_enqueue_decode_finish(st, d_items, count, max_chunks, flags, d_status, d_bad_chunk, d_result, d_scratch);
}

}  // extern "C"
