// snappy_hip_sz_ranges.hip -- the fifth source of libsnappy_hip.so: a resident chunk index of .sz streams and byte ranges decoded
// from it (snappy_sz_ranges.hpp; snappy_hip_sz_index_batch and snappy_hip_sz_decompress_ranges, include/snappy_hip.h).
//
// As snappy_hip_sz_split.hip: a new feature's kernels live in a source of their own.  This one takes the __device__ pieces of the
// other headers without their kernels (SNAPPY_HIP_NO_KERNELS, SNAPPY_SZ_NO_KERNELS), launches only kernels it defines itself, and
// enqueues the split walk of snappy_hip_sz_split.hip through host_shared.hpp.
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
#include "snappy_sz_ranges.hpp"

using namespace snappy_hip_host;

static_assert(sizeof(snappy_hip_sz_chunk) == sizeof(snappy_hip::SzChunk) && sizeof(snappy_hip_sz_chunk) == 32, "snappy_hip_sz_chunk layout");
static_assert(offsetof(snappy_hip_sz_chunk, src_off) == offsetof(snappy_hip::SzChunk, src_off) &&
                  offsetof(snappy_hip_sz_chunk, dst_off) == offsetof(snappy_hip::SzChunk, dst_off) &&
                  offsetof(snappy_hip_sz_chunk, info) == offsetof(snappy_hip::SzChunk, info) &&
                  offsetof(snappy_hip_sz_chunk, ulen) == offsetof(snappy_hip::SzChunk, ulen) &&
                  offsetof(snappy_hip_sz_chunk, item) == offsetof(snappy_hip::SzChunk, item) &&
                  offsetof(snappy_hip_sz_chunk, reserved) == offsetof(snappy_hip::SzChunk, status),
              "snappy_hip_sz_chunk has SzChunk's layout");
static_assert(sizeof(snappy_hip_sz_desc) == sizeof(snappy_hip::SzDesc) && offsetof(snappy_hip_sz_desc, chunks) == offsetof(snappy_hip::SzDesc, chunks) &&
                  offsetof(snappy_hip_sz_desc, total_len) == offsetof(snappy_hip::SzDesc, total_len),
              "snappy_hip_sz_desc layout");
static_assert(sizeof(snappy_hip_range) == sizeof(snappy_hip::RangeDesc), "snappy_hip_range layout");
static_assert(sizeof(snappy_hip_raw_item) == sizeof(snappy_hip::RawItem), "snappy_hip_raw_item layout");

extern "C" {

uint64_t snappy_hip_sz_index_scratch_bytes(uint32_t count, uint32_t max_chunks, uint32_t segment_bytes, uint64_t max_segments)
{
    if (!sz_split_segment_ok(segment_bytes)) return 0;
    return snappy_hip::sz_index_layout(count, sz_split_scratch_total(count, max_chunks, max_segments)).total;
}

int snappy_hip_sz_index_batch(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t max_chunks, uint32_t segment_bytes, uint64_t max_segments,
                              snappy_hip_sz_chunk* d_chunks, snappy_hip_sz_desc* d_descs, uint32_t* d_status, uint32_t* d_result, void* d_scratch,
                              uint64_t scratch_bytes, void* stream)
{
    using namespace snappy_hip;
    if (!sz_split_segment_ok(segment_bytes)) return fail(SNAPPY_HIP_ERR_ARG, "segment_bytes must be 0 or a multiple of 64 of at least 256");
    if (!d_result || (count && (!d_items || !d_descs || !d_status)) || (max_chunks && !d_chunks)) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    max_segments = std::min<uint64_t>(max_segments, 1ull << 31);
    const SzIndexLayout l = sz_index_layout(count, sz_split_scratch_total(count, max_chunks, max_segments));
    if (scratch_bytes < l.total) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_sz_index_scratch_bytes)");
    hipStream_t st = (hipStream_t)stream;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    RawItem* shadow = reinterpret_cast<RawItem*>(scratch);
    uint64_t* out_len = reinterpret_cast<uint64_t*>(scratch + l.out_len);
    uint8_t* split = scratch + l.split;
    const auto* items = reinterpret_cast<const RawItem*>(d_items);
    const uint32_t item_blocks = std::min((std::max(count, 1u) + 255u) / 256u, 1024u);
    if (count) {
        hipLaunchKernelGGL(sz_shadow_items_kernel, dim3(item_blocks), dim3(256), 0, st, items, count, shadow, scratch);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = sz_split_enqueue_walk(st, reinterpret_cast<const snappy_hip_raw_item*>(shadow), count, max_chunks, segment_bytes, max_segments, out_len,
                                       d_status, d_result, split))
        return rc;
    if (count == 0) return SNAPPY_HIP_OK;
    const SzDecodeLayout d = sz_decode_layout(count, max_chunks);
    const uint32_t units = std::max(count, max_chunks);
    hipLaunchKernelGGL(sz_index_export_kernel, dim3(std::min((units + 255u) / 256u, 4096u)), dim3(256), 0, st, items, count,
                       reinterpret_cast<const uint32_t*>(split), reinterpret_cast<const uint64_t*>(split + d.prefix),
                       reinterpret_cast<const SzChunk*>(split + d.chunks), out_len, d_status, reinterpret_cast<SzChunk*>(d_chunks),
                       reinterpret_cast<SzDesc*>(d_descs), d_result);
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}

uint64_t snappy_hip_sz_decompress_ranges_scratch_bytes(uint32_t range_count)
{
    return snappy_hip::sz_range_layout(range_count).slots + (uint64_t)range_grid_cap() * snappy_hip::kSzRangeSlotBytes;
}

int snappy_hip_sz_decompress_ranges(const snappy_hip_sz_desc* d_descs, uint32_t count, const snappy_hip_range* d_ranges, uint32_t range_count,
                                    uint32_t flags, uint32_t* d_status, uint32_t* d_bad_chunk, void* d_scratch, uint64_t scratch_bytes, void* stream)
{
    using namespace snappy_hip;
    if (flags & ~SNAPPY_HIP_SZ_NO_VERIFY) return fail(SNAPPY_HIP_ERR_ARG, "unknown flag (SNAPPY_HIP_SZ_NO_VERIFY is the only one)");
    if (range_count && (!d_ranges || !d_status || !d_bad_chunk || (!d_descs && count))) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    const SzRangeLayout l = sz_range_layout(range_count);
    const uint64_t slots = scratch_bytes > l.slots ? (scratch_bytes - l.slots) / kSzRangeSlotBytes : 0;
    if (slots == 0) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small for one slot (snappy_hip_sz_decompress_ranges_scratch_bytes)");
    if (range_count == 0) return SNAPPY_HIP_OK;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    uint64_t* prefix = reinterpret_cast<uint64_t*>(scratch);
    uint64_t* first = reinterpret_cast<uint64_t*>(scratch + l.first);
    uint64_t* verdict = reinterpret_cast<uint64_t*>(scratch + l.verdict);
    const auto* descs = reinterpret_cast<const SzDesc*>(d_descs);
    const auto* ranges = reinterpret_cast<const RangeDesc*>(d_ranges);
    hipLaunchKernelGGL(sz_range_pieces_kernel, dim3(1), dim3(1024), 0, st, descs, count, ranges, range_count, d_status, prefix, first, verdict);
    HIP_TRY(hipGetLastError());
    const int rc = launch_counted(st, [&](uint32_t* counter) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(range_grid_cap(), slots);
        hipLaunchKernelGGL(sz_decompress_ranges_kernel<kCrcTables>, dim3(grid), dim3(64), 0, st, descs, ranges, range_count, flags, prefix, first, verdict,
                           scratch + l.slots, counter);
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(sz_range_finish_kernel, dim3(std::min((range_count + 255u) / 256u, 4096u)), dim3(256), 0, st, range_count, verdict, d_status,
                       d_bad_chunk);
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}

}  // extern "C"
