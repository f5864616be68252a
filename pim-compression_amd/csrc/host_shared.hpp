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
