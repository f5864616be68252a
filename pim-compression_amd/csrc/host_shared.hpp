// host_shared.hpp -- the host-side helpers that every source of libsnappy_hip.so uses, defined once in snappy_hip.hip: the last
// error, the launch of a persistent kernel on a work counter of its own, and the grid of the persistent decode / check kernels.
// The namespace is hidden: none of this is in the library's dynamic symbol table (tests/test_abi_symbols.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/snappy_hip.h"

namespace snappy_hip_host __attribute__((visibility("hidden"))) {

extern thread_local std::string g_last_error;      // what snappy_hip_last_error() returns

int fail(int code, const std::string& what);       // sets the last error, returns code

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(SNAPPY_HIP_ERR_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

// a zeroed counter for one launch on `st`; call work_counter_launched() right after the launch
struct WorkCounterRing;
struct WorkCounter {
    uint32_t* ptr = nullptr;
    hipEvent_t done = nullptr;
    WorkCounterRing* ring = nullptr;
    uint32_t slot = 0;
};
int next_work_counter(WorkCounter* out, hipStream_t st);
// records the launch's completion event on `st` and releases the slot for reuse behind that event
int work_counter_launched(const WorkCounter& c, hipStream_t st);

// One launch of a persistent kernel on a counter of its own: launch(counter) enqueues the kernel on `st` and returns 0, or
// refuses with fail(...) before it launches anything (the counter is handed back, the refusal is what the caller hears).
// A failure of the counter (taking it, or handing it back) is reported before the launch's own error.
template <class Launch>
int launch_counted(hipStream_t st, Launch launch)
{
    WorkCounter wc;
    if (int rc = next_work_counter(&wc, st)) return rc;
    if (int rc = launch(wc.ptr)) {
        const std::string refusal = g_last_error;
        (void)work_counter_launched(wc, st);
        return fail(rc, refusal);
    }
    const hipError_t launched = hipGetLastError();
    if (int rc = work_counter_launched(wc, st)) return rc;
    HIP_TRY(launched);
    return 0;
}

// wavefronts of a persistent decode / check kernel whose work is counted on the device: K2's grid (SNAPPY_HIP_K2_WAVES)
uint32_t range_grid_cap();

// K1's LDS-table wavefronts outside snappy_hip.hip (the .sz compressor): the refusal of removed knobs (0, or fail(...)), whether
// they run the stream form of the parse at this block size (else the bulk form), and how many of them, with lds_bytes of
// dynamic LDS each, the device holds at once
int check_k1_knobs();
bool lds_table_stream_form(uint32_t block_size);
uint32_t lds_table_resident_waves(uint32_t lds_bytes);

// K1's global-table wavefronts outside snappy_hip.hip (the items' kernel of snappy_hip_items_gt.hip), decided as the container's
// launch decides them for a block size: the slots of the cache in front of the table (512, or 0 = the filter alone), whether
// they run the stream form (else the bulk form), and the launch of one kernel of them over max_fragments fragments with a
// workspace of tables_bytes (launch_shape.hpp: items_gt_small_batch, items_gt_grid; SNAPPY_HIP_GT_WAVES is read per call).
uint32_t global_table_cache_slots(uint32_t block_size);
bool global_table_stream_form(uint32_t block_size);
struct ItemsGtLaunch {
    bool small_batch = false;     // the base call's LDS-table kernel takes the batch
    uint32_t grid = 0;            // else: global-table wavefronts
};
ItemsGtLaunch items_gt_launch(uint32_t block_size, uint32_t max_fragments, uint64_t tables_bytes);

// The steps of snappy_hip_raw_compress_batch, defined in snappy_hip.hip (which owns their kernels) and shared with the call of
// snappy_hip_items_gt.hip that compresses the fragments with a kernel of its own.  raw_compress_check: the call's refusals (0, or
// fail(...) with nothing enqueued).  d_scratch holds raw_layout(count, max_fragments, snappy_hip_slot_stride(block_size)).
// raw_compress_enqueue_plan: raw_plan_kernel.  raw_compress_enqueue_fragments: raw_compress_fragments_kernel, K1's LDS-table form
// (max_fragments != 0).  raw_compress_enqueue_sizes_gather: raw_sizes_kernel (count != 0) and raw_gather_kernel (max_fragments != 0).
// raw_compress_parts: the parts of the scratch a fragment kernel reads and writes -- the control line, the prefix, frag_bytes
// and the slots.
struct CompressParts {
    uint32_t* ctl;
    uint64_t* prefix;
    uint32_t* frag_bytes;
    uint8_t* slots;
};
CompressParts raw_compress_parts(uint32_t count, uint32_t block_size, uint32_t max_fragments, void* d_scratch);
int raw_compress_check(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size, uint32_t max_fragments, const uint64_t* d_out_len,
                       const uint32_t* d_status, const uint32_t* d_result, const void* d_scratch, uint64_t scratch_bytes);
int raw_compress_enqueue_plan(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size, uint32_t max_fragments,
                              uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch);
int raw_compress_enqueue_fragments(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size, uint32_t max_fragments,
                                   void* d_scratch);
int raw_compress_enqueue_sizes_gather(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size, uint32_t max_fragments,
                                      uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch);

// The same for snappy_hip_sz_compress_batch, defined in snappy_hip_sz.hip: d_scratch holds sz_compress_layout(count, max_chunks,
// snappy_hip_slot_stride(chunk_len)).  sz_compress_enqueue_chunks: sz_compress_chunks_kernel, K1's LDS-table form (max_chunks != 0).
// sz_compress_enqueue_crc_sizes_gather: sz_chunk_crc_kernel and sz_gather_kernel (max_chunks != 0) around sz_sizes_kernel (count != 0).
CompressParts sz_compress_parts(uint32_t count, uint32_t chunk_len, uint32_t max_chunks, void* d_scratch);
int sz_compress_check(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks, const uint64_t* d_out_len,
                      const uint32_t* d_status, const uint32_t* d_result, const void* d_scratch, uint64_t scratch_bytes);
int sz_compress_enqueue_plan(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks,
                             uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch);
int sz_compress_enqueue_chunks(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks,
                               void* d_scratch);
int sz_compress_enqueue_crc_sizes_gather(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks,
                                         uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch);

// The steps of snappy_hip_sz_decompress_batch behind its walks, defined in snappy_hip_sz.hip (which owns their kernels) and shared
// with the split walk of snappy_hip_sz_split.hip.  d_scratch starts with the parts of sz_decode_layout(count, max_chunks).
// sz_enqueue_plan: sz_plan_kernel over the items' chunk counts.  sz_enqueue_decode_finish: sz_decode_chunks_kernel over the
// recorded chunks (none with max_chunks == 0), then sz_finish_kernel.  0, or fail(...).
int sz_enqueue_plan(hipStream_t st, uint32_t count, uint32_t max_chunks, uint32_t* d_status, uint32_t* d_result, void* d_scratch);
int sz_enqueue_decode_finish(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t max_chunks, uint32_t flags,
                             uint32_t* d_status, uint32_t* d_bad_chunk, uint32_t* d_result, void* d_scratch);

// Steps 1 to 6 of snappy_hip_sz_decompress_split_batch (snappy_sz_split.hpp: plan, anchors, walkers, join, sz_enqueue_plan, record),
// defined in snappy_hip_sz_split.hip (which owns their kernels) and shared with the index call of snappy_hip_sz_ranges.hip.
// The arguments are validated by the caller: segment_bytes is a good one (not 0), max_segments at most 2^31, d_scratch holds
// sz_split_layout(count, max_chunks, max_segments).  0, or fail(...).
int sz_split_enqueue_walk(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t max_chunks, uint32_t segment_bytes,
                          uint64_t max_segments, uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch);
// segment_bytes 0 becomes the default; whether it is a good one.  The split walk's scratch (sz_split_layout's total).
bool sz_split_segment_ok(uint32_t& segment_bytes);
uint64_t sz_split_scratch_total(uint32_t count, uint32_t max_chunks, uint64_t max_segments);

}  // namespace snappy_hip_host
