// snappy_hip_items_gt.hip -- the sixth source of libsnappy_hip.so: raw and .sz batches compressed by K1's global-table
// wavefronts (snappy_items_gt.hpp; snappy_hip_raw_compress_batch_tables and snappy_hip_sz_compress_batch_tables,
// include/snappy_hip.h).
//
// As snappy_hip_sz_ranges.hip: a new feature's kernel lives in a source of its own.  This one takes the __device__ pieces of the
// other headers without their kernels (SNAPPY_HIP_NO_KERNELS, SNAPPY_SZ_NO_KERNELS), launches only the kernel it defines itself,
// and enqueues the planner, sizes, CRC and gather kernels of the base calls -- and their LDS-table fragment kernels, for a small
// batch -- through host_shared.hpp, from the sources that own them.
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
#include "snappy_sz.hpp"
#include "snappy_items_gt.hpp"

using namespace snappy_hip_host;

static_assert(sizeof(snappy_hip_raw_item) == sizeof(snappy_hip::RawItem), "snappy_hip_raw_item layout");
static_assert((uint32_t)snappy_hip::kSzCtlChunks == (uint32_t)snappy_hip::kRawCtlFragments, "one control word for fragments and chunks");

namespace {

// a null, misaligned or too small table workspace is refused: the call is opt-in
int check_tables(const void* d_tables, uint64_t tables_bytes)
{
    if (!d_tables || ((uintptr_t)d_tables & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_tables must be a 256-byte aligned device pointer");
    if (tables_bytes < 256 + snappy_hip::kItemsGtTableBytes)
        return fail(SNAPPY_HIP_ERR_ARG, "d_tables too small for one table (snappy_hip_compress_scratch_bytes gives the full grid)");
    return 0;
}

// The one kernel of this source over the fragments (or chunks) of a batch whose plan has been enqueued: slot f and frag_bytes[f]
// of the scratch's parts, as the base calls' LDS-table kernels leave them.  The instance is chosen as the container's launch
// chooses its global-table kernel for a block size.
int enqueue_global_table_fragments(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size, uint32_t grid,
                                   const CompressParts& parts, void* d_tables, uint32_t* d_result)
{
    uint32_t* const ctl = parts.ctl;
    uint64_t* const prefix = parts.prefix;
    uint32_t* const frag_bytes = parts.frag_bytes;
    uint8_t* const slots = parts.slots;
    using namespace snappy_hip;
    const auto* items = reinterpret_cast<const RawItem*>(d_items);
    const uint32_t stride = snappy_hip_slot_stride(block_size);
    uint32_t* tables = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(d_tables) + 256);
    const bool cached = global_table_cache_slots(block_size) != 0, stream_form = global_table_stream_form(block_size);
    return launch_counted(st, [&](uint32_t* counter) {
        if (cached && stream_form)
            hipLaunchKernelGGL((item_fragments_global_table_kernel<3, 512>), dim3(grid), dim3(64), 0, st, items, count, block_size, ctl, prefix,
                               frag_bytes, slots, stride, tables, d_result, counter);
        else if (cached)
            hipLaunchKernelGGL((item_fragments_global_table_kernel<2, 512>), dim3(grid), dim3(64), 0, st, items, count, block_size, ctl, prefix,
                               frag_bytes, slots, stride, tables, d_result, counter);
        else if (stream_form)
            hipLaunchKernelGGL((item_fragments_global_table_kernel<3, 0>), dim3(grid), dim3(64), 0, st, items, count, block_size, ctl, prefix,
                               frag_bytes, slots, stride, tables, d_result, counter);
        else
            hipLaunchKernelGGL((item_fragments_global_table_kernel<2, 0>), dim3(grid), dim3(64), 0, st, items, count, block_size, ctl, prefix,
                               frag_bytes, slots, stride, tables, d_result, counter);
        return 0;
    });
}

}  // namespace

extern "C" {

int snappy_hip_raw_compress_batch_tables(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size, uint32_t max_fragments,
                                         uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch, uint64_t scratch_bytes,
                                         void* d_tables, uint64_t tables_bytes, void* stream)
{
    using namespace snappy_hip;
    if (int rc = raw_compress_check(d_items, count, block_size, max_fragments, d_out_len, d_status, d_result, d_scratch, scratch_bytes)) return rc;
    if (int rc = check_tables(d_tables, tables_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_result + 2, 0, 2 * sizeof(uint32_t), st));      // [2]: counted by the kernel below; [3] = 0
    if (int rc = raw_compress_enqueue_plan(st, d_items, count, block_size, max_fragments, d_out_len, d_status, d_result, d_scratch)) return rc;
    if (count && max_fragments) {
        const ItemsGtLaunch launch = items_gt_launch(block_size, max_fragments, tables_bytes);
        if (launch.small_batch) {
            if (int rc = raw_compress_enqueue_fragments(st, d_items, count, block_size, max_fragments, d_scratch)) return rc;
        } else {
            if (int rc = enqueue_global_table_fragments(st, d_items, count, block_size, launch.grid,
                                                        raw_compress_parts(count, block_size, max_fragments, d_scratch), d_tables, d_result))
                return rc;
        }
    }
    return raw_compress_enqueue_sizes_gather(st, d_items, count, block_size, max_fragments, d_out_len, d_status, d_result, d_scratch);
}

int snappy_hip_sz_compress_batch_tables(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks,
                                        uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch, uint64_t scratch_bytes,
                                        void* d_tables, uint64_t tables_bytes, void* stream)
{
    using namespace snappy_hip;
    if (int rc = sz_compress_check(d_items, count, chunk_len, max_chunks, d_out_len, d_status, d_result, d_scratch, scratch_bytes)) return rc;
    if (int rc = check_tables(d_tables, tables_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_result + 2, 0, 2 * sizeof(uint32_t), st));
    if (int rc = sz_compress_enqueue_plan(st, d_items, count, chunk_len, max_chunks, d_out_len, d_status, d_result, d_scratch)) return rc;
    if (count && max_chunks) {
        const ItemsGtLaunch launch = items_gt_launch(chunk_len, max_chunks, tables_bytes);
        if (launch.small_batch) {
            if (int rc = sz_compress_enqueue_chunks(st, d_items, count, chunk_len, max_chunks, d_scratch)) return rc;
        } else {
            if (int rc = enqueue_global_table_fragments(st, d_items, count, chunk_len, launch.grid,
                                                        sz_compress_parts(count, chunk_len, max_chunks, d_scratch), d_tables, d_result))
                return rc;
        }
    }
    return sz_compress_enqueue_crc_sizes_gather(st, d_items, count, chunk_len, max_chunks, d_out_len, d_status, d_result, d_scratch);
}

}  // extern "C"
