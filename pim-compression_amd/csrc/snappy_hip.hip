// snappy_hip.hip -- host side of libsnappy_hip.so: the C ABI declared in include/snappy_hip.h.
//
// Replaces the UPMEM offload plumbing of the reference (dpu_alloc / dpu_load / dpu_push_xfer /
// dpu_launch / dpu_free in snappy/snappy_compress.c:487-714 and snappy/snappy_decompress.c:292-493)
// with hipMalloc / hipMemcpy / kernel launches.  No CPU codec lives in this library: if HIP is
// unusable every entry point fails and says so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/snappy_hip.h"
#include "host_shared.hpp"
#include "shard_devices.hpp"
#include "launch_shape.hpp"
#include "dropin_plan.hpp"
#include "snappy_kernels.hpp"
#include "snappy_ranges.hpp"
#include "snappy_update.hpp"
#include "snappy_raw.hpp"
#include "snappy_raw_split.hpp"
#include "snappy_resize.hpp"
#include "snappy_check.hpp"
#include "snappy_k2_wide.hpp"

namespace snappy_hip_host {   // (shared with the library's other sources: host_shared.hpp)

thread_local std::string g_last_error;

int fail(int code, const std::string& what)
{
    g_last_error = what;
    return code;
}

}  // namespace snappy_hip_host
using namespace snappy_hip_host;

namespace {

double now_seconds()
{
    struct timeval tv;
    gettimeofday(&tv, nullptr);   // same clock as the reference's get_runtime (dpu_snappy.c:87-91)
    return (double)tv.tv_sec + (double)tv.tv_usec / 1000000.0;
}

using dropin_plan::block_size_ok;
using dropin_plan::get_varint32;   // (one home for the varints and the header: csrc/dropin_plan.hpp)
using dropin_plan::put_varint32;

// Run fn(g) for g in [0, count) -- one host thread per device when count > 1 (pageable
// hipMemcpy is synchronous per call, so threads are what overlaps the per-GPU transfers).
int for_each_device(int count, const std::function<int(int)>& fn)
{
    if (count == 1) return fn(0);
    std::vector<int> rc(count, 0);
    std::vector<std::string> err(count);
    std::vector<std::thread> th;
    for (int g = 0; g < count; ++g)
        th.emplace_back([&, g] {
            rc[g] = fn(g);
            if (rc[g]) err[g] = g_last_error;
        });
    for (auto& t : th) t.join();
    for (int g = 0; g < count; ++g)
        if (rc[g]) return fail(rc[g], "GPU " + std::to_string(g) + ": " + err[g]);
    return 0;
}

constexpr int kVariantLdsTable = 1, kVariantGlobalTable = 3;
#ifdef SNAPPY_ABLATION
// The ablation build (tools/build_ablation.py) = the product + ONE experiment kernel: K1 with its hash table answered from
// host-made records (csrc/ablation/k1_oracle_table.hpp, gate (b) of round 4's two-pass question).  The kernel forms of rounds
// 1-3 that do not ship (windowed / masked parses, unfiltered and class-filtered tables, lane-per-block, four blocks per
// wavefront, two-wavefront LDS forms, K2's element loop) were removed in round 4; they are in the history (profiles/HISTORY.md).
constexpr int kVariantOracle = 6, kVariantOracleWithCosts = 7;
const uint32_t* g_oracle_records = nullptr;    // device array, one u32 per input position (tools/gate_b_ceiling.py)
const uint16_t* g_oracle_prevw = nullptr;      // device array, one u16 per input position (variant 7)
#endif
constexpr int kDefaultLdsHeadStart = 6; // ~20 us for the LDS-table workgroups to be placed before the global-table kernel starts
constexpr int kDefaultGtCache = 512;    // SNAPPY_HIP_GT_CACHE: slots of the write-back cache in LDS in front of the global table, for blocks with full-size hash tables; 0 = none
constexpr int kDefaultK1Stream = 1;     // SNAPPY_HIP_K1_STREAM: bit 0 = stream form (snappy_k1_stream.hpp) for the LDS-table kernel (default: +2 % in the mix), bit 1 = for the global-table kernel (default with the slot cache: +3 % there, -2 % without)

// Work counters for persistent kernels: a ring in the code object's own global memory (one copy per device), so launches
// need no allocation.  Each launch takes the next slot of its device's ring, zeroes it on its stream and leaves an event
// behind; a slot is handed out again only after the event of its previous launch has completed (normally long ago: the
// ring has 256 slots), so two launches in flight never share a counter however many streams the caller uses.
constexpr uint32_t kWorkCounterSlots = 256;
__device__ uint32_t g_work_counters[kWorkCounterSlots * 16];      // one counter per 64-byte line

}  // namespace
struct snappy_hip_host::WorkCounterRing {
    std::mutex m;
    uint32_t turn = 0;
    hipEvent_t busy[kWorkCounterSlots] = {};
    bool taken[kWorkCounterSlots] = {};      // handed out, launch event not recorded yet
};
namespace {
WorkCounterRing* work_counter_ring(int dev)
{
    static WorkCounterRing* rings[64] = {};
    static std::mutex m;
    std::lock_guard<std::mutex> lock(m);
    if (!rings[dev]) rings[dev] = new WorkCounterRing;             // never destroyed (threads may outlive statics)
    return rings[dev];
}

}  // namespace

int snappy_hip_host::next_work_counter(WorkCounter* out, hipStream_t st)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(SNAPPY_HIP_ERR_ARG, "device index out of range");
    uint32_t* base = nullptr;
    HIP_TRY(hipGetSymbolAddress((void**)&base, HIP_SYMBOL(g_work_counters)));
    WorkCounterRing* ring = work_counter_ring(dev);
    uint32_t slot;
    hipEvent_t ev;
    {
        std::lock_guard<std::mutex> lock(ring->m);
        uint32_t tries = 0;
        do {
            slot = ring->turn++ % kWorkCounterSlots;
        } while (ring->taken[slot] && ++tries < kWorkCounterSlots);
        if (ring->taken[slot]) return fail(SNAPPY_HIP_ERR_RUNTIME, "all work counters are being launched");
        if (!ring->busy[slot]) HIP_TRY(hipEventCreateWithFlags(&ring->busy[slot], hipEventDisableTiming));
        ring->taken[slot] = true;
        ev = ring->busy[slot];
    }
    out->ptr = base + slot * 16;
    out->done = ev;
    out->ring = ring;
    out->slot = slot;
    hipError_t e = hipEventSynchronize(ev);                        // an event never recorded counts as complete
    if (e == hipSuccess) e = hipMemsetAsync(out->ptr, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) {
        std::lock_guard<std::mutex> lock(ring->m);
        ring->taken[slot] = false;
        return fail(SNAPPY_HIP_ERR_RUNTIME, std::string("work counter: ") + hipGetErrorString(e));
    }
    return 0;
}
int snappy_hip_host::work_counter_launched(const WorkCounter& c, hipStream_t st)
{
    const hipError_t e = hipEventRecord(c.done, st);
    {
        std::lock_guard<std::mutex> lock(c.ring->m);
        c.ring->taken[c.slot] = false;
    }
    if (e != hipSuccess) return fail(SNAPPY_HIP_ERR_RUNTIME, std::string("hipEventRecord: ") + hipGetErrorString(e));
    return 0;
}

namespace {

// Helper stream + fork/join events for launches that co-run two kernels, one set per (host thread, device).  The
// events are timing-disabled; the helper stream is non-blocking, so the only ordering is the explicit fork (ev_begin)
// and join (ev_end) around the caller's stream.
struct CoRunResources {
    hipStream_t helper = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
};

// The sets live in a per-device pool; a host thread leases one per device on first use and hands it back when it ends
// (the drop-in pair runs one short-lived thread per shard), so streams are created once per process, not per call.
struct CoRunPool {
    std::mutex m;
    std::vector<CoRunResources*> idle[64];
};
CoRunPool& corun_pool()
{
    static CoRunPool* pool = new CoRunPool;     // never destroyed: threads may outlive static destruction order
    return *pool;
}
struct CoRunLease {
    CoRunResources* held[64] = {};
    ~CoRunLease()
    {
        CoRunPool& pool = corun_pool();
        std::lock_guard<std::mutex> lock(pool.m);
        for (int d = 0; d < 64; ++d)
            if (held[d]) pool.idle[d].push_back(held[d]);
    }
};

int corun_resources(CoRunResources** out)
{
    static thread_local CoRunLease lease;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(SNAPPY_HIP_ERR_ARG, "device index out of range");
    if (!lease.held[dev]) {
        CoRunPool& pool = corun_pool();
        {
            std::lock_guard<std::mutex> lock(pool.m);
            if (!pool.idle[dev].empty()) {
                lease.held[dev] = pool.idle[dev].back();
                pool.idle[dev].pop_back();
            }
        }
        if (!lease.held[dev]) {
            CoRunResources* r = new CoRunResources;
            HIP_TRY(hipStreamCreateWithFlags(&r->helper, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&r->ev_begin, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&r->ev_end, hipEventDisableTiming));
            lease.held[dev] = r;
        }
    }
    *out = lease.held[dev];
    return 0;
}

int env_int(const char* name, int fallback)
{
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : fallback;
}

// The shape of the current device -- compute units, LDS per CU, wavefront slots per CU -- read once per device.  Every launch
// and the hash-table scratch are sized from it (csrc/launch_shape.hpp), so a partition of the chip (CPX / NPS modes: 32 CUs
// per logical device) gets grids of its own size.  Falls back to a whole MI355X if the runtime cannot be asked.
launch_shape::DeviceShape device_shape()
{
    static std::mutex m;
    static launch_shape::DeviceShape shapes[64];
    static bool known[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return launch_shape::DeviceShape();
    std::lock_guard<std::mutex> lock(m);
    if (!known[dev]) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0 && p.maxSharedMemoryPerMultiProcessor >= (32u << 10) &&
            p.maxThreadsPerMultiProcessor >= 64) {
            shapes[dev].cus = (uint32_t)p.multiProcessorCount;
            shapes[dev].lds_per_cu = (uint32_t)p.maxSharedMemoryPerMultiProcessor;
            shapes[dev].wave_slots_per_cu = (uint32_t)p.maxThreadsPerMultiProcessor / 64u;
        }
        // SNAPPY_HIP_TEST_DEVICE_CUS (test hook, read once per device): pretend the device has this many compute units -- a
        // partition of the chip as CPX / NPS modes make it -- so that the launch and scratch sizing for a small device can be
        // exercised on a whole one (tests/test_gpu_parity.py)
        const int fake = env_int("SNAPPY_HIP_TEST_DEVICE_CUS", 0);
        if (fake > 0 && (uint32_t)fake <= shapes[dev].cus) shapes[dev].cus = (uint32_t)fake;
        known[dev] = true;
    }
    return shapes[dev];
}

using launch_shape::lds_alloc_bytes;

// K1's defaults depend on the block size: blocks of more than 8 KiB have the full 16384-slot table, whose global-table form
// runs at the HBM's random-access rate; there the slot cache and the stream form pay (profiles/r03_gt_cache_block_size_sweep.txt)
int gt_cache_slots(uint32_t block_size)
{
    return env_int("SNAPPY_HIP_GT_CACHE", block_size > 8192u ? kDefaultGtCache : 0) ? 512 : 0;    // (values other than 0 / 512 are refused: check_knobs)
}
int k1_stream_forms(uint32_t block_size)
{
    return env_int("SNAPPY_HIP_K1_STREAM", kDefaultK1Stream | (gt_cache_slots(block_size) ? 2 : 0));
}

// The form of K1's parse the LDS-table wavefronts run at this block size, and the dynamic LDS that goes with it:
// fn(std::integral_constant<int, form>, lds_bytes), form 3 = stream, 2 = bulk (LDS_TABLE_WAVE_COMPRESS, snappy_kernels.hpp)
template <class Fn>
void with_lds_table_form(uint32_t block_size, Fn fn)
{
    if (k1_stream_forms(block_size) & 1) fn(std::integral_constant<int, 3>(), snappy_hip::lds_table_stream_lds_bytes(block_size));
    else fn(std::integral_constant<int, 2>(), snappy_hip::lds_table_kernel_lds_bytes(block_size, true));
}

// dynamic LDS of one LDS-table workgroup of the product's launch at this block size
uint32_t lds_table_wave_bytes(uint32_t block_size)
{
    uint32_t bytes = 0;
    with_lds_table_form(block_size, [&](auto, uint32_t lds) { bytes = lds; });
    return bytes;
}

uint32_t default_lds_waves_per_cu(uint32_t block_size)
{
    launch_shape::K1Knobs k;
    k.cached_global_table = gt_cache_slots(block_size) != 0;
    k.lds_wave_bytes = lds_table_wave_bytes(block_size);
    return launch_shape::default_lds_waves_per_cu(device_shape(), k);
}

// static LDS of one global-table wavefront at this block size: the filter (2 KiB), the scratch of the parse in its form and,
// for blocks with full-size tables, the slot cache
uint32_t global_table_wave_bytes(uint32_t block_size)
{
    const int k1_stream = k1_stream_forms(block_size);
    const int gt_cache = gt_cache_slots(block_size);
    return gt_cache ? ((k1_stream & 2) ? 4u << 10 : 3u << 10) + 4u * (uint32_t)gt_cache
           : (k1_stream & 2) ? (2u << 10) + snappy_hip::stream_scratch_bytes(snappy_hip::kStreamSlotsGlobal)
                             : 3u << 10;
}

// Number of shards the drop-in pair splits a file into: SNAPPY_HIP_NUM_GPUS (default: every visible device).
// SNAPPY_HIP_OVERSUBSCRIBE=1 (test hook) allows more shards than devices; shard g then runs on device
// (base + g) % device_count, so the sharding and host-side concat paths can be exercised on a one-GPU box.
// (ShardDevices -- per call: where the shards of THIS call of the drop-in pair run -- lives in shard_devices.hpp)
ShardDevices requested_devices()
{
    ShardDevices d;
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess || have <= 0) return d;
    d.physical = have;
    int cur = 0;
    if (hipGetDevice(&cur) == hipSuccess && cur > 0 && cur < have) d.base = cur;
    const char* env = getenv("SNAPPY_HIP_NUM_GPUS");
    if (env && *env) {
        const int want = atoi(env);
        const bool over = env_int("SNAPPY_HIP_OVERSUBSCRIBE", 0) != 0;
        if (want >= 1 && (want < have || (over && want <= 64))) have = want;
    }
    d.shards = have;
    return d;
}

// The drop-in pair leaves the calling thread's current device as it found it (its shard threads are its own).
struct CallerDevice {
    int dev = -1;
    CallerDevice()
    {
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    }
    ~CallerDevice()
    {
        if (dev >= 0) (void)hipSetDevice(dev);
    }
};

// K1 launchers: the LDS-table kernel and the global-table kernel, each in the bulk or the stream form of the parse, the
// global-table one behind its slot cache for blocks with full-size hash tables.

// Knobs of earlier rounds' kernel forms, and values of the product's own knobs that no build implements any more, are
// refused, not ignored: a sweep must never produce numbers labelled with a configuration that did not run.
int check_knobs()
{
    for (const char* name : {"SNAPPY_HIP_K1_AHEAD", "SNAPPY_HIP_K1_AHEAD_LDS", "SNAPPY_HIP_K1_FORM", "SNAPPY_HIP_K1_FORM_LDS",
                             "SNAPPY_HIP_K1_FILTER", "SNAPPY_HIP_EXTRA_LDS", "SNAPPY_HIP_LANES_PER_BLOCK", "SNAPPY_HIP_GROUP_WAVES",
                             "SNAPPY_HIP_PAIR_PER_CU"})
        if (getenv(name))
            return fail(SNAPPY_HIP_ERR_ARG, std::string(name) + " selected a kernel form of rounds 1-3 that was removed in round 4 "
                                                                "(profiles/HISTORY.md names the commit that has them)");
    if (const char* v = getenv("SNAPPY_HIP_GT_CACHE"))
        if (*v && atoi(v) != 0 && atoi(v) != 512)
            return fail(SNAPPY_HIP_ERR_ARG, "SNAPPY_HIP_GT_CACHE: the slot cache has 512 slots or is off (0)");
    if (const char* v = getenv("SNAPPY_HIP_K1_STREAM"))
        if (*v && (atoi(v) & ~3))
            return fail(SNAPPY_HIP_ERR_ARG, "SNAPPY_HIP_K1_STREAM: bits 0 and 1 select the stream form per kernel (bit 2, round 3's duo form, was removed)");
    return 0;
}

void launch_lds_table_kernel(uint32_t grid, hipStream_t st, const snappy_hip::K1Batch& w, uint32_t block_size, uint32_t slot_stride,
                             uint32_t* counter)
{
    with_lds_table_form(block_size, [&](auto form, uint32_t lds) {
        hipLaunchKernelGGL((snappy_hip::compress_blocks_lds_table_kernel<64, form()>), dim3(grid), dim3(64), lds, st, w, block_size, slot_stride,
                           counter);
    });
}

void launch_global_table_kernel(uint32_t grid, hipStream_t st, const snappy_hip::K1Batch& w, uint32_t block_size, uint32_t slot_stride,
                                uint32_t* tables, uint32_t* counter)
{
    const bool cached = gt_cache_slots(block_size) != 0;
    const bool stream_form = (k1_stream_forms(block_size) & 2) != 0;
    if (cached && stream_form)
        hipLaunchKernelGGL((snappy_hip::compress_blocks_global_table_kernel<64, 3, 1, 512>), dim3(grid), dim3(64), 0, st, w, block_size,
                           slot_stride, tables, counter);
    else if (cached)
        hipLaunchKernelGGL((snappy_hip::compress_blocks_global_table_kernel<64, 2, 1, 512>), dim3(grid), dim3(64), 0, st, w, block_size,
                           slot_stride, tables, counter);
    else if (stream_form)
        hipLaunchKernelGGL((snappy_hip::compress_blocks_global_table_kernel<64, 3, 1>), dim3(grid), dim3(64), 0, st, w, block_size,
                           slot_stride, tables, counter);
    else
        hipLaunchKernelGGL((snappy_hip::compress_blocks_global_table_kernel<64, 2, 1>), dim3(grid), dim3(64), 0, st, w, block_size,
                           slot_stride, tables, counter);
}

}  // namespace

namespace {

// Workspace of the parallel-segment chain resolution (csrc/snappy_kernels.hpp: chain_*_kernel), one per device, owned by the
// library: 2.1 MB per stream of a call, allocated on first use and when a call brings more streams than any before it (the
// only moment snappy_hip_index_streams touches the allocator).  Calls that overlap in time on different streams are ordered
// by an event: the later one waits ON THE DEVICE for the earlier one to be done with the workspace.
struct ChainWorkspace {
    std::mutex m;
    uint32_t* mem = nullptr;
    uint32_t streams = 0;
    hipEvent_t last_use = nullptr;
};
ChainWorkspace* chain_workspace(int dev)
{
    static ChainWorkspace* per_device[64] = {};
    static std::mutex m;
    std::lock_guard<std::mutex> lock(m);
    if (!per_device[dev]) per_device[dev] = new ChainWorkspace;    // never destroyed (threads may outlive statics)
    return per_device[dev];
}

}  // namespace

// ===========================================================================
// resident API
// ===========================================================================
extern "C" {

void* snappy_hip_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) {
        g_last_error = "hipHostMalloc failed";
        return nullptr;
    }
    return p;
}

void snappy_hip_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

int snappy_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        g_last_error = "hipGetDeviceCount failed: no usable HIP runtime/device";
        return 0;
    }
    return n;
}

int snappy_hip_set_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return SNAPPY_HIP_OK;
}

const char* snappy_hip_last_error(void) { return g_last_error.c_str(); }

const char* snappy_hip_arch(void) { return "gfx950"; }

uint32_t snappy_hip_slot_stride(uint32_t block_size)
{
    const uint64_t need = 4ull + 32ull + block_size + block_size / 6;   // snappy_compress.c:55-60 + prefix
    return (uint32_t)((need + 15) & ~15ull);
}

uint64_t snappy_hip_num_blocks(uint64_t input_len, uint32_t block_size)
{
    return block_size ? (input_len + block_size - 1) / block_size : 0;
}

uint64_t snappy_hip_stream_bound(uint64_t input_len, uint32_t block_size)
{
    return 10 + snappy_hip_num_blocks(input_len, block_size) * (uint64_t)snappy_hip_slot_stride(block_size);
}

uint32_t snappy_hip_write_header(uint8_t* dst, uint32_t total_len, uint32_t block_size)
{
    uint32_t k = put_varint32(dst, total_len);
    k += put_varint32(dst + k, block_size);
    return k;
}

uint32_t snappy_hip_parse_header(const uint8_t* src, uint64_t avail, uint32_t* total_len, uint32_t* block_size)
{
    return dropin_plan::parse_header(src, avail, total_len, block_size);
}

#ifdef SNAPPY_ABLATION
// ablation build only: the records OracleTable / RecMate read (csrc/ablation/k1_oracle_table.hpp)
void snappy_hip_debug_set_oracle_records(const uint32_t* d_records) { g_oracle_records = d_records; }
void snappy_hip_debug_set_oracle_prevw(const uint16_t* d_prevw) { g_oracle_prevw = d_prevw; }
#endif

#ifdef SNAPPY_PROF
// probe builds only (tools/prof_stream.py): read / reset the lap timers of the stream form
int snappy_hip_debug_prof(unsigned long long* out, int reset)
{
    if (reset) {
        unsigned long long z[32] = {0};
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(snappy_hip::g_prof), z, sizeof(z));
    }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(snappy_hip::g_prof), 32 * sizeof(unsigned long long));
}
#endif

uint32_t snappy_hip_k1_lds_waves_per_cu(uint32_t block_size)
{
    if (!block_size_ok(block_size)) return 0;
    const launch_shape::DeviceShape shape = device_shape();
    const int forced = env_int("SNAPPY_HIP_LDS_WAVES", -1);
    return forced >= 0 ? ((uint32_t)forced + shape.cus - 1) / shape.cus : default_lds_waves_per_cu(block_size);
}

uint64_t snappy_hip_compress_scratch_bytes(void)
{
    // 256-byte header (work counter) + one 64 KiB hash table per wavefront slot of the CURRENT device (MI355X: 256 CUs x 32)
    return launch_shape::compress_scratch_bytes(device_shape());
}

// K1 over a batch of containers (count >= 1, every container non-empty and validated by the callers below)
static int launch_compress(const snappy_hip::K1Batch& w, uint32_t block_size, uint32_t slot_stride, void* d_scratch,
                           uint64_t scratch_bytes, void* stream)
{
    const uint64_t nb = w.first_block[w.count];
    // SNAPPY_HIP_COMPRESS_VARIANT: 3 = the concurrent launch below (default); 1 = the LDS-table kernel alone (also the path
    // taken when no scratch is given); the ablation build has 6 = the free-table experiment (csrc/ablation/k1_oracle_table.hpp).
    int variant = env_int("SNAPPY_HIP_COMPRESS_VARIANT", kVariantGlobalTable);
    if (variant == kVariantGlobalTable &&
        (!d_scratch || scratch_bytes < snappy_hip_compress_scratch_bytes() || ((uintptr_t)d_scratch & 255)))
        variant = kVariantLdsTable;   // no scratch: LDS-table kernel (still on the GPU)
    if (int rc = check_knobs()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const launch_shape::DeviceShape shape = device_shape();
    const bool scratch_usable = d_scratch && scratch_bytes >= 256 && !((uintptr_t)d_scratch & 255);
    // A small input -- every block can have an LDS-table wavefront at once, at most one per SIMD -- goes to the LDS-table
    // kernel alone: its wavefronts run the stream form with nothing else on their SIMD (dickens_like, 312 blocks: K1 1.27 ->
    // 1.05 ms, profiles/r03_small_inputs.txt); with more blocks than that a second round would follow, and the global-table
    // kernel's 32 wave slots per CU win.
    if (variant == kVariantGlobalTable && !getenv("SNAPPY_HIP_COMPRESS_VARIANT") && !getenv("SNAPPY_HIP_LDS_WAVES") &&
        (k1_stream_forms(block_size) & 1) &&
        launch_shape::small_input_takes_lds_kernel_alone(shape, snappy_hip::lds_table_stream_lds_bytes(block_size), nb))
        variant = kVariantLdsTable;
#ifdef SNAPPY_ABLATION
    if (variant == kVariantOracle || variant == kVariantOracleWithCosts) {     // ceiling experiment (csrc/ablation/k1_oracle_table.hpp)
        const bool costs = variant == kVariantOracleWithCosts;
        if (w.count != 1 || !g_oracle_records || !d_scratch ||
            (costs && (!g_oracle_prevw || scratch_bytes < snappy_hip_compress_scratch_bytes() || block_size > 32768u)))
            return fail(SNAPPY_HIP_ERR_ARG, "variants 6 / 7 take one container, a scratch and snappy_hip_debug_set_oracle_records() (7: + _prevw())");
        uint32_t* counter = static_cast<uint32_t*>(d_scratch);
        uint16_t* memo = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(d_scratch) + 256);
        HIP_TRY(hipMemsetAsync(counter, 0, 32, st));
        const uint32_t waves = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(nb, shape.wave_slots()), (uint64_t)env_int("SNAPPY_HIP_GT_WAVES", (int)(20 * shape.cus)));
        if (costs)
            hipLaunchKernelGGL(snappy_hip::compress_blocks_oracle_kernel<true>, dim3(waves), dim3(64), 0, st, w, block_size, slot_stride,
                               g_oracle_records, g_oracle_prevw, memo, counter);
        else
            hipLaunchKernelGGL(snappy_hip::compress_blocks_oracle_kernel<false>, dim3(waves), dim3(64), 0, st, w, block_size, slot_stride,
                               g_oracle_records, g_oracle_prevw, memo, counter);
        HIP_TRY(hipGetLastError());
        return SNAPPY_HIP_OK;
    }
#endif
    if (variant != kVariantGlobalTable && variant != kVariantLdsTable)
        return fail(SNAPPY_HIP_ERR_ARG, "SNAPPY_HIP_COMPRESS_VARIANT: 1 (LDS-table kernel alone) or 3 (the concurrent launch, default)");
    if (variant == kVariantLdsTable) {
        launch_lds_table_kernel((uint32_t)nb, st, w, block_size, slot_stride, (uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
        // the statistics word of the scratch (include/snappy_hip.h): every block of this launch had an LDS-table wavefront
        if (scratch_usable) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(static_cast<uint32_t*>(d_scratch) + 4), (int)nb, 1, st));
        return SNAPPY_HIP_OK;
    }

    // ---- the default: persistent grids, blocks handed out by an atomic counter kept in the first bytes of the scratch ----
    // Wave budget per CU (MI355X: 256 CUs, 32 wave slots, 160 KiB of LDS each; device_shape()): a global-table wavefront holds
    // the duplicate test, the slot filter (2 KiB) and, for blocks with full-size tables, the slot cache (2 KiB) in LDS and its
    // table in the scratch; the wavefronts whose table lives in LDS are sized by the block length (csrc/launch_shape.hpp).
    // SNAPPY_HIP_LDS_WAVES overrides the LDS-table wavefronts, SNAPPY_HIP_GT_WAVES the TOTAL of both kinds.
    uint32_t* counter = static_cast<uint32_t*>(d_scratch);
    uint32_t* tables = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(d_scratch) + 256);
    HIP_TRY(hipMemsetAsync(counter, 0, 32, st));   // [0] next block, [4] blocks compressed by wavefronts with an LDS table
    launch_shape::K1Knobs knobs;
    knobs.cached_global_table = gt_cache_slots(block_size) != 0;
    knobs.lds_wave_bytes = lds_table_wave_bytes(block_size);
    knobs.gt_wave_bytes = global_table_wave_bytes(block_size);
    knobs.lds_waves_forced = env_int("SNAPPY_HIP_LDS_WAVES", -1);
    knobs.waves_forced = env_int("SNAPPY_HIP_GT_WAVES", -1);
    knobs.hybrid_min_blocks = (uint64_t)env_int("SNAPPY_HIP_HYBRID_MIN_BLOCKS", 4096);     // small inputs: one kernel is enough
    const launch_shape::K1Launch l = launch_shape::k1_default_launch(shape, knobs, nb);
    if (l.lds_waves) {
        // fork / join around the caller's stream: the LDS-table kernel goes to the helper stream, the global-table kernel stays
        // on `st`; both draw blocks from the same counter, so the split balances itself
        CoRunResources* cr = nullptr;
        if (int rc = corun_resources(&cr)) return rc;
        HIP_TRY(hipEventRecord(cr->ev_begin, st));                     // after the counter memset and all prior work
        HIP_TRY(hipStreamWaitEvent(cr->helper, cr->ev_begin, 0));
        launch_lds_table_kernel(l.lds_waves, cr->helper, w, block_size, slot_stride, counter);
        HIP_TRY(hipEventRecord(cr->ev_end, cr->helper));
        // a head start for the LDS-heavy workgroups: placed first, the small allocations cannot fragment the LDS under them
        if (const int head_start = env_int("SNAPPY_HIP_LDS_HEAD_START", kDefaultLdsHeadStart))   // x 3.4 us
            hipLaunchKernelGGL(snappy_hip::delay_kernel, dim3(1), dim3(64), 0, st, (uint32_t)head_start);
        launch_global_table_kernel(l.gt_waves, st, w, block_size, slot_stride, tables, counter);
        HIP_TRY(hipStreamWaitEvent(st, cr->ev_end, 0));                // the caller's stream resumes when both are done
    } else {
        launch_global_table_kernel(l.gt_waves, st, w, block_size, slot_stride, tables, counter);
    }
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}

static int check_container(const void* d_in, uint64_t input_len, uint32_t block_size, const void* d_slots, uint32_t slot_stride,
                           const void* d_block_bytes)
{
    if (!block_size_ok(block_size)) return fail(SNAPPY_HIP_ERR_ARG, "block_size must be 1..65535");
    if (input_len > 0xffffffffull) return fail(SNAPPY_HIP_ERR_ARG, "container length must fit uint32 (snappy_compress.c:461)");
    if (slot_stride < snappy_hip_slot_stride(block_size)) return fail(SNAPPY_HIP_ERR_ARG, "slot_stride too small");
    if (((uintptr_t)d_in & 15) || ((uintptr_t)d_slots & 15)) return fail(SNAPPY_HIP_ERR_ARG, "d_in and d_slots must be 16-byte aligned");
    if (input_len && (!d_in || !d_slots || !d_block_bytes)) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    return SNAPPY_HIP_OK;
}

int snappy_hip_compress_blocks(const uint8_t* d_in, uint64_t input_len, uint32_t block_size, uint8_t* d_slots,
                               uint32_t slot_stride, uint32_t* d_block_bytes, void* d_scratch, uint64_t scratch_bytes,
                               void* stream)
{
    if (int rc = check_container(d_in, input_len, block_size, d_slots, slot_stride, d_block_bytes)) return rc;
    const uint64_t nb = snappy_hip_num_blocks(input_len, block_size);
    if (nb == 0) return SNAPPY_HIP_OK;
    snappy_hip::K1Batch w{};
    w.count = 1;
    w.first_block[0] = 0;
    w.first_block[1] = (uint32_t)nb;
    w.in[0] = d_in;
    w.in_len[0] = input_len;
    w.slots[0] = d_slots;
    w.block_bytes[0] = d_block_bytes;
    return launch_compress(w, block_size, slot_stride, d_scratch, scratch_bytes, stream);
}

int snappy_hip_compress_blocks_batch(const struct snappy_hip_compress_item* items, uint32_t count, uint32_t block_size,
                                     uint32_t slot_stride, void* d_scratch, uint64_t scratch_bytes, void* stream)
{
    if (!items && count) return fail(SNAPPY_HIP_ERR_ARG, "null item array");
    // empty containers are skipped; a launch takes at most kMaxBatch non-empty ones, so longer lists go out in groups
    uint32_t i = 0;
    while (i < count) {
        snappy_hip::K1Batch w{};
        uint64_t blocks = 0;
        while (i < count && w.count < snappy_hip::kMaxBatch) {
            const snappy_hip_compress_item& it = items[i];
            if (int rc = check_container(it.d_input, it.input_len, block_size, it.d_slots, slot_stride, it.d_block_bytes)) return rc;
            const uint64_t nb = snappy_hip_num_blocks(it.input_len, block_size);
            if (nb) {
                if (blocks + nb > 0xffffffffull) break;
                w.first_block[w.count] = (uint32_t)blocks;
                w.in[w.count] = static_cast<const uint8_t*>(it.d_input);
                w.in_len[w.count] = it.input_len;
                w.slots[w.count] = static_cast<uint8_t*>(it.d_slots);
                w.block_bytes[w.count] = static_cast<uint32_t*>(it.d_block_bytes);
                blocks += nb;
                ++w.count;
            }
            ++i;
        }
        w.first_block[w.count] = (uint32_t)blocks;
        if (w.count)
            if (int rc = launch_compress(w, block_size, slot_stride, d_scratch, scratch_bytes, stream)) return rc;
    }
    return SNAPPY_HIP_OK;
}

int snappy_hip_compact(const uint8_t* d_slots, uint32_t slot_stride, const uint32_t* d_block_bytes, uint64_t input_len,
                       uint32_t block_size, uint8_t* d_stream, uint64_t* d_offsets, uint64_t* d_stream_len, void* stream)
{
    if (!block_size_ok(block_size)) return fail(SNAPPY_HIP_ERR_ARG, "block_size must be 1..65535");
    if (input_len > 0xffffffffull) return fail(SNAPPY_HIP_ERR_ARG, "container length must fit uint32");
    if (!d_stream || !d_offsets) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    const uint32_t nb = (uint32_t)snappy_hip_num_blocks(input_len, block_size);
    hipLaunchKernelGGL(snappy_hip::scan_block_bytes_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, d_block_bytes, nb,
                       (uint32_t)input_len, block_size, d_stream, d_offsets, d_stream_len);
    HIP_TRY(hipGetLastError());
    if (nb) {
        hipLaunchKernelGGL(snappy_hip::gather_slots_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, d_slots, slot_stride,
                           d_block_bytes, d_offsets, d_stream, nb);
        HIP_TRY(hipGetLastError());
    }
    return SNAPPY_HIP_OK;
}

int snappy_hip_index_streams(const snappy_hip_stream_desc* d_descs, uint32_t count, void* stream)
{
    static_assert(sizeof(snappy_hip_stream_desc) == sizeof(snappy_hip::StreamDesc), "descriptor layout");
    if (count == 0) return SNAPPY_HIP_OK;
    if (!d_descs) return fail(SNAPPY_HIP_ERR_ARG, "null descriptor array");
    hipStream_t st = (hipStream_t)stream;
    const snappy_hip::StreamDesc* dd = reinterpret_cast<const snappy_hip::StreamDesc*>(d_descs);
    // SNAPPY_HIP_INDEX_READERS=0: the walking wavefront alone, without the read-ahead workgroups on its XCD
    const uint32_t group = env_int("SNAPPY_HIP_INDEX_READERS", 1) ? snappy_hip::kIndexGroup : 1u;
    // SNAPPY_HIP_INDEX_PARALLEL=0: the serial walk only (the parallel segments resolve a stream or leave it to that walk)
    if (!env_int("SNAPPY_HIP_INDEX_PARALLEL", 1)) {
        hipLaunchKernelGGL(snappy_hip::index_streams_kernel, dim3(count * group), dim3(64 * snappy_hip::kIndexWgWaves), 0, st, dd, count,
                           group, (const uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
        return SNAPPY_HIP_OK;
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(SNAPPY_HIP_ERR_ARG, "device index out of range");
    ChainWorkspace* cw = chain_workspace(dev);
    std::lock_guard<std::mutex> lock(cw->m);
    constexpr size_t kSegs = snappy_hip::kChainSegments, kCap = snappy_hip::kChainSegCap;
    const size_t words_per_stream = kSegs * (3 + kCap) + 1;
    if (cw->streams < count) {
        if (cw->last_use) HIP_TRY(hipEventSynchronize(cw->last_use));
        if (cw->mem) (void)hipFree(cw->mem);
        cw->mem = nullptr;
        cw->streams = 0;
        HIP_TRY(hipMalloc((void**)&cw->mem, (size_t)count * words_per_stream * sizeof(uint32_t)));
        cw->streams = count;
    }
    if (!cw->last_use) HIP_TRY(hipEventCreateWithFlags(&cw->last_use, hipEventDisableTiming));
    HIP_TRY(hipStreamWaitEvent(st, cw->last_use, 0));             // (an event never recorded counts as complete)
    snappy_hip::ChainWork w;
    w.anchor = cw->mem;
    w.seg_hops = w.anchor + (size_t)count * kSegs;
    w.seg_ok = w.seg_hops + (size_t)count * kSegs;
    w.hops = w.seg_ok + (size_t)count * kSegs;
    w.resolved = w.hops + (size_t)count * kSegs * kCap;
    hipLaunchKernelGGL(snappy_hip::chain_anchor_kernel, dim3(count * (uint32_t)kSegs), dim3(64), 0, st, dd, count, w);
    hipLaunchKernelGGL(snappy_hip::chain_walk_kernel, dim3(count * (uint32_t)kSegs), dim3(64), 0, st, dd, count, w);
    hipLaunchKernelGGL(snappy_hip::chain_finish_kernel, dim3(count), dim3(1024), 0, st, dd, count, w);
    hipLaunchKernelGGL(snappy_hip::index_streams_kernel, dim3(count * group), dim3(64 * snappy_hip::kIndexWgWaves), 0, st, dd, count, group,
                       (const uint32_t*)w.resolved);
    const hipError_t launched = hipGetLastError();
    HIP_TRY(hipEventRecord(cw->last_use, st));
    HIP_TRY(launched);
    return SNAPPY_HIP_OK;
}

int snappy_hip_verify_index(const snappy_hip_stream_desc* d_descs, uint32_t count, void* stream)
{
    if (count == 0) return SNAPPY_HIP_OK;
    if (!d_descs) return fail(SNAPPY_HIP_ERR_ARG, "null descriptor array");
    const snappy_hip::StreamDesc* dd = reinterpret_cast<const snappy_hip::StreamDesc*>(d_descs);
    hipLaunchKernelGGL(snappy_hip::verify_index_begin_kernel, dim3((count + 63) / 64), dim3(64), 0, (hipStream_t)stream, dd, count);
    hipLaunchKernelGGL(snappy_hip::verify_index_kernel, dim3(count * snappy_hip::kVerifyGroup), dim3(256), 0, (hipStream_t)stream,
                       dd, count);
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}

// K2 over a batch of streams (count >= 1, every stream non-empty and validated by the callers below)
static int launch_decompress(const snappy_hip::K2Batch& w, uint32_t block_size, void* stream)
{
    const uint64_t nb = w.first_block[w.count];
    hipStream_t st = (hipStream_t)stream;
    // every block's status starts as "not decoded": a block the launch never reaches cannot read back as OK
    for (uint32_t c = 0; c < w.count; ++c)
        HIP_TRY(hipMemsetAsync(w.status[c], 0xff, (size_t)(w.first_block[c + 1] - w.first_block[c]) * sizeof(uint32_t), st));
    return launch_counted(st, [&](uint32_t* counter) {
        const launch_shape::DeviceShape shape = device_shape();
        const uint32_t k2_cap = (uint32_t)std::max(1, env_int("SNAPPY_HIP_K2_WAVES", (int)shape.wave_slots()));   // fewer wavefronts leave slots for a co-running kernel
        if (getenv("SNAPPY_HIP_DECOMPRESS_VARIANT") || getenv("SNAPPY_HIP_K2_BATCH") || getenv("SNAPPY_HIP_K2_LDS_WAVES"))
            return fail(SNAPPY_HIP_ERR_ARG, "SNAPPY_HIP_DECOMPRESS_VARIANT / SNAPPY_HIP_K2_BATCH / SNAPPY_HIP_K2_LDS_WAVES selected decoder forms of "
                                            "rounds 1-2 that were removed in round 4 (profiles/HISTORY.md)");
        hipLaunchKernelGGL(snappy_hip::decompress_blocks_kernel, dim3(launch_shape::k2_launch_waves(shape, nb, (int)k2_cap)), dim3(64), 0, st, w,
                           block_size, counter);
        return 0;
    });
}

static int check_stream(const void* d_stream, const void* d_block_offsets, uint64_t total_len, uint32_t block_size, const void* d_out,
                        const void* d_status)
{
    if (!block_size_ok(block_size)) return fail(SNAPPY_HIP_ERR_ARG, "block_size must be 1..65535");
    if (total_len && (!d_stream || !d_block_offsets || !d_out || !d_status)) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (snappy_hip_num_blocks(total_len, block_size) > 0x7fffffffull) return fail(SNAPPY_HIP_ERR_ARG, "too many blocks");
    return SNAPPY_HIP_OK;
}

int snappy_hip_decompress_blocks(const uint8_t* d_stream, uint64_t stream_len, const uint64_t* d_block_offsets,
                                 uint64_t total_len, uint32_t block_size, uint8_t* d_out, uint32_t* d_status, void* stream)
{
    if (total_len == 0) return SNAPPY_HIP_OK;
    if (int rc = check_stream(d_stream, d_block_offsets, total_len, block_size, d_out, d_status)) return rc;
    snappy_hip::K2Batch w{};
    w.count = 1;
    w.first_block[0] = 0;
    w.first_block[1] = (uint32_t)snappy_hip_num_blocks(total_len, block_size);
    w.stream[0] = d_stream;
    w.stream_len[0] = stream_len;
    w.block_offsets[0] = d_block_offsets;
    w.total_len[0] = total_len;
    w.out[0] = d_out;
    w.status[0] = d_status;
    return launch_decompress(w, block_size, stream);
}

int snappy_hip_decompress_blocks_batch(const struct snappy_hip_decompress_item* items, uint32_t count, uint32_t block_size, void* stream)
{
    if (!items && count) return fail(SNAPPY_HIP_ERR_ARG, "null item array");
    // empty streams are skipped; a launch takes at most kMaxBatch non-empty ones, so longer lists go out in groups
    uint32_t i = 0;
    while (i < count) {
        snappy_hip::K2Batch w{};
        uint64_t blocks = 0;
        while (i < count && w.count < snappy_hip::kMaxBatch) {
            const snappy_hip_decompress_item& it = items[i];
            if (int rc = check_stream(it.d_stream, it.d_block_offsets, it.total_len, block_size, it.d_out, it.d_status)) return rc;
            const uint64_t nb = snappy_hip_num_blocks(it.total_len, block_size);
            if (nb) {
                if (blocks + nb > 0x7fffffffull) break;
                w.first_block[w.count] = (uint32_t)blocks;
                w.stream[w.count] = static_cast<const uint8_t*>(it.d_stream);
                w.stream_len[w.count] = it.stream_len;
                w.stream_len_dev[w.count] = static_cast<const uint64_t*>(it.d_stream_len);
                w.block_offsets[w.count] = static_cast<const uint64_t*>(it.d_block_offsets);
                w.total_len[w.count] = it.total_len;
                w.out[w.count] = static_cast<uint8_t*>(it.d_out);
                w.status[w.count] = static_cast<uint32_t*>(it.d_status);
                blocks += nb;
                ++w.count;
            }
            ++i;
        }
        w.first_block[w.count] = (uint32_t)blocks;
        if (w.count)
            if (int rc = launch_decompress(w, block_size, stream)) return rc;
    }
    return SNAPPY_HIP_OK;
}

// ---- one block on a whole workgroup (snappy_k2_wide.hpp) ----
static_assert(SNAPPY_HIP_WIDE_MAX_BLOCK == snappy_hip::kWideMaxBlock && SNAPPY_HIP_WIDE_MAX_CSZ == snappy_hip::kWideMaxCsz, "the wide path's limits");
static_assert(SNAPPY_HIP_WIDE_MAX_CSZ >= 32u + 32768u + 32768u / 6u, "every compressor-made block of at most 32 KiB is within the limits");

int snappy_hip_decompress_blocks_wide(const uint8_t* d_stream, uint64_t stream_len, const uint64_t* d_block_offsets, uint64_t total_len,
                                      uint32_t block_size, uint8_t* d_out, uint32_t* d_status, uint32_t waves_per_block, uint32_t* d_result,
                                      void* stream)
{
    if (waves_per_block == 0) waves_per_block = snappy_hip::kWideMaxWaves;
    if (waves_per_block != 2 && waves_per_block != 4 && waves_per_block != 8 && waves_per_block != 16)
        return fail(SNAPPY_HIP_ERR_ARG, "waves_per_block must be 0, 2, 4, 8 or 16");
    if (!d_result) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (total_len)
        if (int rc = check_stream(d_stream, d_block_offsets, total_len, block_size, d_out, d_status)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_result, 0, 4 * sizeof(uint32_t), st));
    if (total_len == 0) return SNAPPY_HIP_OK;
    const uint32_t nb = (uint32_t)snappy_hip_num_blocks(total_len, block_size);
    // every block's status starts as "not decoded", as K2's launch has it
    HIP_TRY(hipMemsetAsync(d_status, 0xff, (size_t)nb * sizeof(uint32_t), st));
    return launch_counted(st, [&](uint32_t* counter) {
        // one workgroup per CU (its LDS is most of a CU's); SNAPPY_HIP_K2_WAVES caps the grid, the unit being workgroups here
        const launch_shape::DeviceShape shape = device_shape();
        const uint32_t cap = (uint32_t)std::max(1, env_int("SNAPPY_HIP_K2_WAVES", (int)shape.cus));
        const uint32_t grid = std::min(std::min(nb, shape.cus), cap);
        hipLaunchKernelGGL(snappy_hip::k2_wide_kernel, dim3(grid), dim3(64 * waves_per_block), 0, st, d_stream, stream_len, d_block_offsets, total_len,
                           block_size, d_out, d_status, nb, d_result, counter);
        return 0;
    });
}

// ---- byte ranges (snappy_ranges.hpp) ----
}  // extern "C"
uint32_t snappy_hip_host::range_grid_cap()
{
    const launch_shape::DeviceShape shape = device_shape();
    const int cap = std::max(1, env_int("SNAPPY_HIP_K2_WAVES", (int)shape.wave_slots()));
    return launch_shape::k2_launch_waves(shape, ~0ull, cap);
}
int snappy_hip_host::check_k1_knobs() { return check_knobs(); }
bool snappy_hip_host::lds_table_stream_form(uint32_t block_size) { return (k1_stream_forms(block_size) & 1) != 0; }
uint32_t snappy_hip_host::lds_table_resident_waves(uint32_t lds_bytes) { return launch_shape::update_resident_waves(device_shape(), lds_bytes); }
uint32_t snappy_hip_host::global_table_cache_slots(uint32_t block_size) { return (uint32_t)gt_cache_slots(block_size); }
bool snappy_hip_host::global_table_stream_form(uint32_t block_size) { return (k1_stream_forms(block_size) & 2) != 0; }
snappy_hip_host::ItemsGtLaunch snappy_hip_host::items_gt_launch(uint32_t block_size, uint32_t max_fragments, uint64_t tables_bytes)
{
    const launch_shape::DeviceShape shape = device_shape();
    launch_shape::K1Knobs knobs;
    knobs.cached_global_table = gt_cache_slots(block_size) != 0;
    knobs.lds_wave_bytes = lds_table_wave_bytes(block_size);
    knobs.gt_wave_bytes = global_table_wave_bytes(block_size);
    knobs.waves_forced = env_int("SNAPPY_HIP_GT_WAVES", -1);
    ItemsGtLaunch l;
    l.small_batch = launch_shape::items_gt_small_batch(shape, knobs, max_fragments);
    l.grid = launch_shape::items_gt_grid(shape, knobs, max_fragments, tables_bytes);
    return l;
}
extern "C" {

uint64_t snappy_hip_decompress_ranges_scratch_bytes(uint32_t max_block_size, uint32_t range_count)
{
    if (!block_size_ok(max_block_size)) return 0;
    return snappy_hip::range_prefix_bytes(range_count) + (uint64_t)range_grid_cap() * snappy_hip::range_slot_bytes(max_block_size);
}

int snappy_hip_decompress_ranges(const snappy_hip_stream_desc* d_descs, uint32_t count, const snappy_hip_range* d_ranges, uint32_t range_count,
                                 uint32_t* d_status, uint32_t max_block_size, void* d_scratch, uint64_t scratch_bytes, void* stream)
{
    static_assert(sizeof(snappy_hip_range) == sizeof(snappy_hip::RangeDesc), "snappy_hip_range layout");
    static_assert(sizeof(snappy_hip_stream_desc) == sizeof(snappy_hip::StreamDesc), "snappy_hip_stream_desc layout");
    if (range_count == 0) return SNAPPY_HIP_OK;
    if (!block_size_ok(max_block_size)) return fail(SNAPPY_HIP_ERR_ARG, "max_block_size must be 1..65535");
    if (!d_ranges || !d_status || (!d_descs && count)) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    const uint64_t prefix_bytes = snappy_hip::range_prefix_bytes(range_count), slot_bytes = snappy_hip::range_slot_bytes(max_block_size);
    const uint64_t slots = scratch_bytes > prefix_bytes ? (scratch_bytes - prefix_bytes) / slot_bytes : 0;
    if (slots == 0) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small for one slot (snappy_hip_decompress_ranges_scratch_bytes)");
    hipStream_t st = (hipStream_t)stream;
    uint64_t* prefix = static_cast<uint64_t*>(d_scratch);
    uint8_t* slot_base = static_cast<uint8_t*>(d_scratch) + prefix_bytes;
    const auto* descs = reinterpret_cast<const snappy_hip::StreamDesc*>(d_descs);
    const auto* ranges = reinterpret_cast<const snappy_hip::RangeDesc*>(d_ranges);
    hipLaunchKernelGGL(snappy_hip::range_pieces_kernel, dim3(1), dim3(1024), 0, st, descs, count, ranges, range_count, d_status, max_block_size,
                       prefix);
    HIP_TRY(hipGetLastError());
    return launch_counted(st, [&](uint32_t* counter) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(range_grid_cap(), slots);
        hipLaunchKernelGGL(snappy_hip::decompress_ranges_kernel, dim3(grid), dim3(64), 0, st, descs, ranges, range_count, d_status, prefix,
                           slot_base, (uint32_t)slot_bytes, counter);
        return 0;
    });
}

// ---- overwriting byte ranges (snappy_update.hpp) ----
// dynamic LDS and wavefronts of the recompress kernel: the LDS-table kernel's form and LDS at this block size, plus K2's stage
static uint32_t update_grid_cap(uint32_t block_size)
{
    return launch_shape::update_resident_waves(device_shape(), snappy_hip::kK2StageBytes + lds_table_wave_bytes(block_size));
}

uint64_t snappy_hip_update_scratch_bytes(uint32_t block_size, uint32_t num_blocks, uint32_t write_count, uint32_t max_dirty_blocks)
{
    (void)write_count;      // (the writes are searched where they are; no scratch per write)
    if (!block_size_ok(block_size)) return 0;
    const uint32_t waves = std::max(1u, std::min(update_grid_cap(block_size), max_dirty_blocks));
    return snappy_hip::update_layout(block_size, num_blocks, max_dirty_blocks, waves, snappy_hip_slot_stride(block_size)).total;
}

int snappy_hip_update_ranges(const snappy_hip_stream_desc* d_desc, uint32_t total_len, uint32_t block_size, const snappy_hip_write* d_writes,
                             uint32_t write_count, uint32_t* d_write_status, uint8_t* d_new_stream, uint64_t new_stream_capacity,
                             uint64_t* d_new_offsets, uint64_t* d_new_stream_len, uint32_t* d_result, uint32_t max_dirty_blocks,
                             void* d_scratch, uint64_t scratch_bytes, void* stream)
{
    static_assert(sizeof(snappy_hip_write) == sizeof(snappy_hip::WriteDesc), "snappy_hip_write layout");
    if (!block_size_ok(block_size)) return fail(SNAPPY_HIP_ERR_ARG, "block_size must be 1..65535");
    if (!d_desc || !d_new_stream || !d_new_offsets || !d_new_stream_len || !d_result || (write_count && (!d_writes || !d_write_status)))
        return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (write_count && max_dirty_blocks == 0) return fail(SNAPPY_HIP_ERR_ARG, "max_dirty_blocks must not be 0 when there are writes");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    const uint32_t nb = (uint32_t)snappy_hip_num_blocks(total_len, block_size);
    const uint32_t stride = snappy_hip_slot_stride(block_size);
    const uint32_t waves = std::max(1u, std::min(update_grid_cap(block_size), max_dirty_blocks));
    const snappy_hip::UpdateLayout l = snappy_hip::update_layout(block_size, nb, max_dirty_blocks, waves, stride);
    if (scratch_bytes < l.total) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_update_scratch_bytes)");
    if (int rc = check_knobs()) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(scratch);
    uint32_t* span = reinterpret_cast<uint32_t*>(scratch + l.span);
    uint32_t* rank = reinterpret_cast<uint32_t*>(scratch + l.rank);
    uint32_t* dirty = reinterpret_cast<uint32_t*>(scratch + l.dirty);
    uint32_t* dirty_bytes = reinterpret_cast<uint32_t*>(scratch + l.dirty_bytes);
    const auto* desc = reinterpret_cast<const snappy_hip::StreamDesc*>(d_desc);
    const auto* writes = reinterpret_cast<const snappy_hip::WriteDesc*>(d_writes);
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));
    if (nb)
        hipLaunchKernelGGL(snappy_hip::update_mark_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, desc, total_len, block_size, nb, writes,
                           write_count, ctl, span);
    hipLaunchKernelGGL(snappy_hip::update_plan_kernel, dim3(1), dim3(1024), 0, st, desc, total_len, block_size, nb, writes, write_count,
                       d_write_status, max_dirty_blocks, ctl, span, rank, dirty, d_new_stream_len, d_result);
    HIP_TRY(hipGetLastError());
    if (write_count && nb) {
        const int rc = launch_counted(st, [&](uint32_t* counter) {
            with_lds_table_form(block_size, [&](auto form, uint32_t lds) {
                hipLaunchKernelGGL(snappy_hip::recompress_dirty_kernel<form()>, dim3(waves), dim3(64), lds, st, desc, total_len, block_size, writes,
                                   write_count, ctl, dirty, dirty_bytes, scratch + l.patch, l.patch_slot_bytes, scratch + l.cslots, stride, counter);
            });
            return 0;
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(snappy_hip::update_sizes_kernel, dim3(1), dim3(1024), 0, st, total_len, block_size, nb, ctl, span, rank, dirty_bytes,
                       d_new_stream, new_stream_capacity, d_new_offsets, d_new_stream_len, d_result);
    if (nb)
        hipLaunchKernelGGL(snappy_hip::merge_stream_kernel, dim3(nb), dim3(256), 0, st, desc, nb, ctl, rank, scratch + l.cslots, stride,
                           d_new_offsets, d_new_stream);
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}

// ---- growing and shrinking a container (snappy_resize.hpp) ----
// the shape of one resize: blocks of the new container, those of them that are compressed, wavefronts of the recompress kernel
struct ResizeShape {
    uint32_t new_blocks, compressed, waves;
};
static ResizeShape resize_shape(uint32_t block_size, uint32_t new_total_len, uint32_t keep_len)
{
    ResizeShape s;
    s.new_blocks = (uint32_t)snappy_hip_num_blocks(new_total_len, block_size);
    const uint32_t kept = keep_len / block_size;
    s.compressed = s.new_blocks > kept ? s.new_blocks - kept : 0;      // (keep_len > new_total_len is REJECTED on the device)
    s.waves = std::max(1u, std::min(update_grid_cap(block_size), s.compressed));
    return s;
}

uint64_t snappy_hip_resize_scratch_bytes(uint32_t block_size, uint32_t old_num_blocks, uint32_t new_total_len, uint32_t keep_len,
                                         uint32_t segment_count)
{
    (void)old_num_blocks;   // (a kept block is a block of the new container too: nothing is sized by the old count)
    if (!block_size_ok(block_size)) return 0;
    const ResizeShape s = resize_shape(block_size, new_total_len, keep_len);
    return snappy_hip::resize_layout(block_size, s.new_blocks, s.compressed, segment_count, s.waves, snappy_hip_slot_stride(block_size)).total;
}

int snappy_hip_resize(const snappy_hip_stream_desc* d_desc, uint32_t total_len, uint32_t block_size, uint32_t keep_len, uint32_t new_total_len,
                      const snappy_hip_segment* d_segments, uint32_t segment_count, uint32_t* d_segment_status, uint8_t* d_new_stream,
                      uint64_t new_stream_capacity, uint64_t* d_new_offsets, uint64_t* d_new_stream_len, uint32_t* d_result, void* d_scratch,
                      uint64_t scratch_bytes, void* stream)
{
    static_assert(sizeof(snappy_hip_segment) == sizeof(snappy_hip::SegmentDesc) && sizeof(snappy_hip::SegmentDesc) == 16, "snappy_hip_segment layout");
    if (!block_size_ok(block_size)) return fail(SNAPPY_HIP_ERR_ARG, "block_size must be 1..65535");
    if (!d_desc || !d_new_stream || !d_new_offsets || !d_new_stream_len || !d_result || (segment_count && (!d_segments || !d_segment_status)))
        return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    const uint32_t nb = (uint32_t)snappy_hip_num_blocks(total_len, block_size);
    const uint32_t stride = snappy_hip_slot_stride(block_size);
    const ResizeShape s = resize_shape(block_size, new_total_len, keep_len);
    const snappy_hip::ResizeLayout l = snappy_hip::resize_layout(block_size, s.new_blocks, s.compressed, segment_count, s.waves, stride);
    if (scratch_bytes < l.total) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_resize_scratch_bytes)");
    if (int rc = check_knobs()) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(scratch);
    uint64_t* prefix = reinterpret_cast<uint64_t*>(scratch + l.prefix);
    uint32_t* span = reinterpret_cast<uint32_t*>(scratch + l.span);
    uint32_t* rank = reinterpret_cast<uint32_t*>(scratch + l.rank);
    uint32_t* new_bytes = reinterpret_cast<uint32_t*>(scratch + l.new_bytes);
    const auto* desc = reinterpret_cast<const snappy_hip::StreamDesc*>(d_desc);
    const auto* segments = reinterpret_cast<const snappy_hip::SegmentDesc*>(d_segments);
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));
    if (s.new_blocks)
        hipLaunchKernelGGL(snappy_hip::resize_mark_kernel, dim3((uint32_t)(((uint64_t)s.new_blocks + 255) / 256)), dim3(256), 0, st, desc, total_len,
                           block_size, nb, keep_len, s.new_blocks, ctl, span, rank);
    hipLaunchKernelGGL(snappy_hip::resize_plan_kernel, dim3(1), dim3(1024), 0, st, desc, total_len, block_size, nb, keep_len, new_total_len,
                       s.new_blocks, segments, segment_count, d_segment_status, ctl, prefix, d_new_stream_len, d_result);
    HIP_TRY(hipGetLastError());
    if (s.compressed) {
        const int rc = launch_counted(st, [&](uint32_t* counter) {
            with_lds_table_form(block_size, [&](auto form, uint32_t lds) {
                hipLaunchKernelGGL(snappy_hip::resize_recompress_kernel<form()>, dim3(s.waves), dim3(64), lds, st, desc, total_len, block_size, keep_len,
                                   new_total_len, segments, segment_count, prefix, ctl, new_bytes, scratch + l.patch, l.patch_slot_bytes,
                                   scratch + l.cslots, stride, counter);
            });
            return 0;
        });
        if (rc) return rc;
    }
    // a kept block is the update's clean block, new block kept + k its dirty block k: the same sizes, scan, header and merge
    hipLaunchKernelGGL(snappy_hip::update_sizes_kernel, dim3(1), dim3(1024), 0, st, new_total_len, block_size, s.new_blocks, ctl, span, rank,
                       new_bytes, d_new_stream, new_stream_capacity, d_new_offsets, d_new_stream_len, d_result);
    if (s.new_blocks)
        hipLaunchKernelGGL(snappy_hip::merge_stream_kernel, dim3(std::min(s.new_blocks, 0x7fffffffu)), dim3(256), 0, st, desc, s.new_blocks, ctl, rank,
                           scratch + l.cslots, stride, d_new_offsets, d_new_stream);
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}

// ---- batches of raw Snappy streams (snappy_raw.hpp) ----
int snappy_hip_raw_decompress_batch(const snappy_hip_raw_item* d_items, uint32_t count, uint64_t* d_out_len, uint32_t* d_status, void* stream)
{
    static_assert(sizeof(snappy_hip_raw_item) == sizeof(snappy_hip::RawItem) && sizeof(snappy_hip::RawItem) == 32, "snappy_hip_raw_item layout");
    static_assert(SNAPPY_HIP_RAW_MAX_LEN == snappy_hip::kRawMaxLen && SNAPPY_HIP_RAW_MAX_LEN >= (1ull << 30), "SNAPPY_HIP_RAW_MAX_LEN");
    static_assert(SNAPPY_HIP_RAW_DST_TOO_SMALL == snappy_hip::kRawDstTooSmall && SNAPPY_HIP_RAW_TOO_LARGE == snappy_hip::kRawTooLarge, "raw status codes");
    if (count == 0) return SNAPPY_HIP_OK;
    if (!d_items || !d_out_len || !d_status) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    hipStream_t st = (hipStream_t)stream;
    return launch_counted(st, [&](uint32_t* counter) {
        const uint32_t grid = std::min(range_grid_cap(), count);
        hipLaunchKernelGGL(snappy_hip::raw_decompress_kernel, dim3(grid), dim3(64), 0, st, reinterpret_cast<const snappy_hip::RawItem*>(d_items), count,
                           d_out_len, d_status, counter);
        return 0;
    });
}

uint64_t snappy_hip_raw_compress_bound(uint64_t src_len, uint32_t block_size)
{
    if (!block_size_ok(block_size)) return 0;
    // per fragment of n bytes K1 writes at most 32 + n + n / 6 bytes of elements (what snappy_hip_slot_stride reserves)
    const uint64_t fragments = snappy_hip_num_blocks(src_len, block_size);
    return 5 + fragments * 32 + src_len + src_len / 6;
}

uint64_t snappy_hip_raw_compress_scratch_bytes(uint32_t block_size, uint32_t count, uint32_t max_fragments)
{
    if (!block_size_ok(block_size)) return 0;
    return snappy_hip::raw_layout(count, max_fragments, snappy_hip_slot_stride(block_size)).total;
}

int snappy_hip_raw_compress_batch(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size, uint32_t max_fragments,
                                  uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch, uint64_t scratch_bytes,
                                  void* stream)
{
    if (int rc = raw_compress_check(d_items, count, block_size, max_fragments, d_out_len, d_status, d_result, d_scratch, scratch_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = raw_compress_enqueue_plan(st, d_items, count, block_size, max_fragments, d_out_len, d_status, d_result, d_scratch)) return rc;
    if (count && max_fragments)
        if (int rc = raw_compress_enqueue_fragments(st, d_items, count, block_size, max_fragments, d_scratch)) return rc;
    return raw_compress_enqueue_sizes_gather(st, d_items, count, block_size, max_fragments, d_out_len, d_status, d_result, d_scratch);
}

}  // extern "C"
// (host_shared.hpp: the steps of the call above, shared with snappy_hip_items_gt.hip)
namespace {
struct RawCompressParts {
    const snappy_hip::RawItem* items;
    uint32_t stride;
    snappy_hip::RawLayout l;
    uint8_t* scratch;
    uint32_t* ctl;
    uint64_t* prefix;
    uint32_t* frag_bytes;
    uint64_t* place;
    RawCompressParts(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size, uint32_t max_fragments, void* d_scratch)
        : items(reinterpret_cast<const snappy_hip::RawItem*>(d_items)), stride(snappy_hip_slot_stride(block_size)),
          l(snappy_hip::raw_layout(count, max_fragments, stride)), scratch(static_cast<uint8_t*>(d_scratch)), ctl(reinterpret_cast<uint32_t*>(scratch)),
          prefix(reinterpret_cast<uint64_t*>(scratch + l.prefix)), frag_bytes(reinterpret_cast<uint32_t*>(scratch + l.frag_bytes)),
          place(reinterpret_cast<uint64_t*>(scratch + l.place))
    {
    }
};
}  // namespace
snappy_hip_host::CompressParts snappy_hip_host::raw_compress_parts(uint32_t count, uint32_t block_size, uint32_t max_fragments, void* d_scratch)
{
    const RawCompressParts p(nullptr, count, block_size, max_fragments, d_scratch);
    return CompressParts{p.ctl, p.prefix, p.frag_bytes, p.scratch + p.l.slots};
}
int snappy_hip_host::raw_compress_check(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size, uint32_t max_fragments,
                                        const uint64_t* d_out_len, const uint32_t* d_status, const uint32_t* d_result, const void* d_scratch,
                                        uint64_t scratch_bytes)
{
    if (!block_size_ok(block_size)) return fail(SNAPPY_HIP_ERR_ARG, "block_size must be 1..65535");
    if (!d_result || (count && (!d_items || !d_out_len || !d_status))) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    const snappy_hip::RawLayout l = snappy_hip::raw_layout(count, max_fragments, snappy_hip_slot_stride(block_size));
    if (scratch_bytes < l.total) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_raw_compress_scratch_bytes)");
    return check_knobs();
}
int snappy_hip_host::raw_compress_enqueue_plan(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size,
                                               uint32_t max_fragments, uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch)
{
    const RawCompressParts p(d_items, count, block_size, max_fragments, d_scratch);
    hipLaunchKernelGGL(snappy_hip::raw_plan_kernel, dim3(1), dim3(1024), 0, st, p.items, count, block_size, max_fragments, d_out_len, d_status,
                       d_result, p.ctl, p.prefix);
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}
int snappy_hip_host::raw_compress_enqueue_fragments(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size,
                                                    uint32_t max_fragments, void* d_scratch)
{
    const RawCompressParts p(d_items, count, block_size, max_fragments, d_scratch);
    return launch_counted(st, [&](uint32_t* counter) {
        with_lds_table_form(block_size, [&](auto form, uint32_t lds) {
            const uint32_t waves = std::min(launch_shape::update_resident_waves(device_shape(), lds), max_fragments);
            hipLaunchKernelGGL(snappy_hip::raw_compress_fragments_kernel<form()>, dim3(waves), dim3(64), lds, st, p.items, count, block_size, p.ctl,
                               p.prefix, p.frag_bytes, p.scratch + p.l.slots, p.stride, counter);
        });
        return 0;
    });
}
int snappy_hip_host::raw_compress_enqueue_sizes_gather(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t block_size,
                                                       uint32_t max_fragments, uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result,
                                                       void* d_scratch)
{
    const RawCompressParts p(d_items, count, block_size, max_fragments, d_scratch);
    if (count)      // (without a slot only empty items can be OK)
        hipLaunchKernelGGL(snappy_hip::raw_sizes_kernel, dim3(std::min(count, 4096u)), dim3(64), 0, st, p.items, count, p.prefix, p.frag_bytes, p.place,
                           d_out_len, d_status, d_result);
    if (count && max_fragments)
        hipLaunchKernelGGL(snappy_hip::raw_gather_kernel, dim3(std::min(max_fragments, 32768u)), dim3(256), 0, st, p.items, count, p.ctl, p.prefix,
                           p.frag_bytes, p.place, p.scratch + p.l.slots, p.stride, d_status);
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}
extern "C" {

// ---- one large raw stream over many wavefronts (snappy_raw_split.hpp) ----
static bool split_params(uint32_t& unit_len, uint32_t& segment_bytes)
{
    if (unit_len == 0) unit_len = snappy_hip::kSplitDefaultUnit;
    if (segment_bytes == 0) segment_bytes = snappy_hip::kSplitDefaultSegment;
    return unit_len >= 256u && segment_bytes >= 128u && segment_bytes % 64u == 0;
}

uint64_t snappy_hip_raw_decompress_split_scratch_bytes(uint32_t count, uint32_t unit_len, uint32_t segment_bytes, uint64_t max_segments,
                                                       uint64_t max_units)
{
    if (!split_params(unit_len, segment_bytes)) return 0;
    return snappy_hip::split_layout(count, max_segments, max_units).total;
}

int snappy_hip_raw_decompress_split_batch(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t unit_len, uint32_t segment_bytes,
                                          uint64_t max_segments, uint64_t max_units, uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result,
                                          void* d_scratch, uint64_t scratch_bytes, void* stream)
{
    using namespace snappy_hip;
    if (!split_params(unit_len, segment_bytes))
        return fail(SNAPPY_HIP_ERR_ARG, "unit_len must be 0 or at least 256, segment_bytes 0 or a multiple of 64 of at least 128");
    if (!d_result || (count && (!d_items || !d_out_len || !d_status))) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    max_segments = std::min(max_segments, kSplitMaxWork);
    max_units = std::min(max_units, kSplitMaxWork);
    const SplitLayout l = split_layout(count, max_segments, max_units);
    if (scratch_bytes < l.total) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_raw_decompress_split_scratch_bytes)");
    hipStream_t st = (hipStream_t)stream;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(scratch);
    uint64_t* seg_prefix = reinterpret_cast<uint64_t*>(scratch + l.seg_prefix);
    uint64_t* unit_prefix = reinterpret_cast<uint64_t*>(scratch + l.unit_prefix);
    uint32_t* flags = reinterpret_cast<uint32_t*>(scratch + l.flags);
    uint64_t* table = reinterpret_cast<uint64_t*>(scratch + l.table);
    uint4* nodes = reinterpret_cast<uint4*>(scratch + l.nodes);
    uint32_t* cuts = reinterpret_cast<uint32_t*>(scratch + l.cuts);
    const auto* items = reinterpret_cast<const RawItem*>(d_items);
    hipLaunchKernelGGL(raw_split_plan_kernel, dim3(1), dim3(1024), 0, st, items, count, unit_len, segment_bytes, max_segments, max_units, d_out_len,
                       d_status, d_result, ctl, seg_prefix, unit_prefix, flags, cuts);
    HIP_TRY(hipGetLastError());
    if (count == 0) return SNAPPY_HIP_OK;
    const uint32_t cap = range_grid_cap();
    if (max_segments && max_units) {        // (else no item can be split: the serial step takes them all)
        const uint32_t seg_grid = (uint32_t)std::min<uint64_t>(cap, max_segments), unit_grid = (uint32_t)std::min<uint64_t>(cap, max_units);
        int rc = launch_counted(st, [&](uint32_t* counter) {
            hipLaunchKernelGGL(raw_split_walk_kernel, dim3(seg_grid), dim3(64), 0, st, items, count, segment_bytes, ctl, seg_prefix, flags, table, nodes,
                               counter);
            return 0;
        });
        if (rc) return rc;
        hipLaunchKernelGGL(raw_split_resolve_kernel, dim3(std::min(count, 4096u)), dim3(64), 0, st, items, count, unit_len, segment_bytes, d_out_len,
                           seg_prefix, unit_prefix, flags, table, nodes, cuts);
        HIP_TRY(hipGetLastError());
        rc = launch_counted(st, [&](uint32_t* counter) {
            hipLaunchKernelGGL(raw_split_cuts_kernel, dim3(seg_grid), dim3(64), 0, st, items, count, unit_len, ctl, d_out_len, seg_prefix, unit_prefix,
                               flags, nodes, cuts, counter);
            return 0;
        });
        if (rc) return rc;
        rc = launch_counted(st, [&](uint32_t* counter) {
            hipLaunchKernelGGL(raw_split_units_kernel, dim3(unit_grid), dim3(64), 0, st, items, count, unit_len, ctl, d_out_len, unit_prefix, flags, cuts,
                               counter);
            return 0;
        });
        if (rc) return rc;
    }
    return launch_counted(st, [&](uint32_t* counter) {
        hipLaunchKernelGGL(raw_split_serial_kernel, dim3(std::min(cap, count)), dim3(64), 0, st, items, count, d_out_len, d_status, flags, d_result,
                           counter);
        return 0;
    });
}

// ---- checking without decoding (snappy_check.hpp) ----
uint64_t snappy_hip_check_scratch_bytes(uint32_t count) { return snappy_hip::check_prefix_bytes(count); }

int snappy_hip_check_blocks(const snappy_hip_stream_desc* d_descs, uint32_t count, uint32_t* const* d_block_status, uint32_t* d_results,
                            void* d_scratch, uint64_t scratch_bytes, void* stream)
{
    static_assert(sizeof(snappy_hip_stream_desc) == sizeof(snappy_hip::StreamDesc), "snappy_hip_stream_desc layout");
    if (count == 0) return SNAPPY_HIP_OK;
    if (!d_descs || !d_results) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    if (scratch_bytes < snappy_hip::check_prefix_bytes(count)) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_check_scratch_bytes)");
    hipStream_t st = (hipStream_t)stream;
    uint64_t* prefix = static_cast<uint64_t*>(d_scratch);
    const auto* descs = reinterpret_cast<const snappy_hip::StreamDesc*>(d_descs);
    hipLaunchKernelGGL(snappy_hip::check_plan_kernel, dim3(1), dim3(1024), 0, st, descs, count, d_results, prefix);
    HIP_TRY(hipGetLastError());
    return launch_counted(st, [&](uint32_t* counter) {
        // the blocks are counted on the device, so the grid is K2's for an unbounded count
        hipLaunchKernelGGL(snappy_hip::check_kernel, dim3(range_grid_cap()), dim3(64), 0, st, descs, count, d_block_status, d_results, prefix, counter);
        return 0;
    });
}

int snappy_hip_raw_check_batch(const snappy_hip_raw_item* d_items, uint32_t count, uint64_t* d_out_len, uint32_t* d_status, void* stream)
{
    if (count == 0) return SNAPPY_HIP_OK;
    if (!d_items || !d_out_len || !d_status) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    hipStream_t st = (hipStream_t)stream;
    return launch_counted(st, [&](uint32_t* counter) {
        const uint32_t grid = std::min(range_grid_cap(), count);
        hipLaunchKernelGGL(snappy_hip::raw_check_kernel, dim3(grid), dim3(64), 0, st, reinterpret_cast<const snappy_hip::RawItem*>(d_items), count,
                           d_out_len, d_status, counter);
        return 0;
    });
}

#ifdef SNAPPY_PAIR_PROBE
int snappy_hip_debug_pair_prof(unsigned long long* out, int reset)
{
    if (reset) {
        unsigned long long z[16] = {0};
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(snappy_hip::g_pair_prof), z, sizeof(z));
    }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(snappy_hip::g_pair_prof), 16 * sizeof(unsigned long long));
}
#endif

}  // extern "C"

#include "dropin_pair.hpp"
