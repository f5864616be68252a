// snappy_hip_raw_check_split.hip -- the second source of libsnappy_hip.so: the split check of raw Snappy streams
// (snappy_raw_check_split.hpp; snappy_hip_raw_check_split_batch, include/snappy_hip.h).
//
// The kernels of snappy_hip.hip are held, instruction for instruction, to what they were measured with, and its tests count
// them; a new feature's kernels therefore live in a source of their own.  This one takes the __device__ pieces of the other
// headers without their kernels (SNAPPY_HIP_NO_KERNELS), launches only kernels it defines itself, and shares the host-side
// helpers of snappy_hip.hip through host_shared.hpp.
#define SNAPPY_HIP_NO_KERNELS
#undef SNAPPY_PROF          // (the probe builds' counters are snappy_hip.hip's own)
#undef SNAPPY_PAIR_PROBE
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/snappy_hip.h"
#include "host_shared.hpp"
#include "snappy_raw_check_split.hpp"

using namespace snappy_hip_host;

static bool vsplit_params(uint32_t& segment_bytes)
{
    if (segment_bytes == 0) segment_bytes = snappy_hip::kSplitDefaultSegment;
    return segment_bytes >= 128u && segment_bytes % 64u == 0;
}

extern "C" {

uint64_t snappy_hip_raw_check_split_scratch_bytes(uint32_t count, uint32_t segment_bytes, uint64_t max_segments)
{
    if (!vsplit_params(segment_bytes)) return 0;
    return snappy_hip::vsplit_layout(count, max_segments).total;
}

int snappy_hip_raw_check_split_batch(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t segment_bytes, uint64_t max_segments,
                                     uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch, uint64_t scratch_bytes,
                                     void* stream)
{
    using namespace snappy_hip;
    static_assert(sizeof(snappy_hip_raw_item) == sizeof(RawItem), "snappy_hip_raw_item layout");
    if (!vsplit_params(segment_bytes)) return fail(SNAPPY_HIP_ERR_ARG, "segment_bytes must be 0 or a multiple of 64 of at least 128");
    if (!d_result || (count && (!d_items || !d_out_len || !d_status))) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    max_segments = std::min(max_segments, kSplitMaxWork);
    const VsplitLayout l = vsplit_layout(count, max_segments);
    if (scratch_bytes < l.total) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_raw_check_split_scratch_bytes)");
    hipStream_t st = (hipStream_t)stream;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(scratch);
    uint64_t* seg_prefix = reinterpret_cast<uint64_t*>(scratch + l.seg_prefix);
    uint32_t* flags = reinterpret_cast<uint32_t*>(scratch + l.flags);
    uint64_t* table = reinterpret_cast<uint64_t*>(scratch + l.table);
    uint4* nodes = reinterpret_cast<uint4*>(scratch + l.nodes);
    const auto* items = reinterpret_cast<const RawItem*>(d_items);
    hipLaunchKernelGGL(raw_vsplit_plan_kernel, dim3(1), dim3(1024), 0, st, items, count, segment_bytes, max_segments, d_out_len, d_status, d_result,
                       ctl, seg_prefix, flags);
    HIP_TRY(hipGetLastError());
    if (count == 0) return SNAPPY_HIP_OK;
    const uint32_t cap = range_grid_cap();
    if (max_segments) {                     // (else no item can be spread: the serial step takes them all)
        const uint32_t seg_grid = (uint32_t)std::min<uint64_t>(cap, max_segments);
        int rc = launch_counted(st, [&](uint32_t* counter) {
            hipLaunchKernelGGL(raw_vsplit_walk_kernel, dim3(seg_grid), dim3(64), 0, st, items, count, segment_bytes, ctl, seg_prefix, flags, table, nodes,
                               counter);
            return 0;
        });
        if (rc) return rc;
        hipLaunchKernelGGL(raw_vsplit_resolve_kernel, dim3(std::min(count, 4096u)), dim3(64), 0, st, items, count, segment_bytes, d_out_len, seg_prefix,
                           flags, table, nodes);
        HIP_TRY(hipGetLastError());
        rc = launch_counted(st, [&](uint32_t* counter) {
            hipLaunchKernelGGL(raw_vsplit_verify_kernel, dim3(seg_grid), dim3(64), 0, st, items, count, segment_bytes, ctl, d_out_len, seg_prefix, flags,
                               nodes, counter);
            return 0;
        });
        if (rc) return rc;
    }
    return launch_counted(st, [&](uint32_t* counter) {
        hipLaunchKernelGGL(raw_vsplit_serial_kernel, dim3(std::min(cap, count)), dim3(64), 0, st, items, count, d_out_len, d_status, flags, d_result,
                           counter);
        return 0;
    });
}

}  // extern "C"
