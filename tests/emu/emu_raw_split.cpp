// The split decode of raw Snappy streams (pim-compression_amd/csrc/snappy_raw_split.hpp) on the CPU wave emulator: a library
// of its own, built by tests/emu_raw_split_lib.py.  Test infrastructure only.
#include "emu_runtime.cpp"
#include "snappy_raw_split.hpp"

#include <memory>

namespace {

constexpr uint8_t kDstFill = 0xEE;           // what every dst holds before the kernels run
constexpr uint8_t kScratchJunk = 0xCD;       // ... and the scratch, and the 256 bytes behind it
constexpr int kWroteBehindScratch = 101;

// What steps 1-4 left in the scratch, for tests/raw_split_cases.model to be held against.  plan_flags / flags: every item's
// flag word after step 1 / after step 4.  For every item the plan classed split inside the limits: count[2 * i] = its units
// + 1 cuts, copied to cuts + cut_at, count[2 * i + 1] = its segments, whose nodes go to nodes + node_at as (entry, landing,
// output base) triples; 0 and 0 for every other item.  cut_room / node_room: words the two arrays hold.
struct SplitTrace {
    uint32_t* plan_flags;
    uint32_t* flags;
    uint32_t* count;
    uint32_t* cuts;
    uint64_t cut_room;
    uint32_t* nodes;
    uint64_t node_room;
};

}  // namespace

extern "C" unsigned emu_raw_split_dst_fill() { return kDstFill; }

// The six kernels as snappy_hip_raw_decompress_split_batch enqueues them, `grid` wavefronts in every persistent one.  Every
// item's src is copied to end at an inaccessible page (real_len[i] bytes are there; src_len[i] is what the item claims) and
// every dst is a window of exactly capacity[i] bytes between inaccessible pages, filled with kDstFill; out[i]: the whole window
// afterwards.  flags bit 0: src is null; bit 1: dst is null.  unit_len and segment_bytes: as the call takes them behind its
// defaults.  The scratch starts out as junk.  Returns 0, or 100 if a kernel wrote in front of a window; a write behind a
// window or a read behind a stream faults: call from a child process.
static int run_split(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity,
                             const uint32_t* flags, uint32_t count, uint32_t unit_len, uint32_t segment_bytes, uint64_t max_segments,
                     uint64_t max_units, uint8_t* const* out, uint64_t* out_len, uint32_t* status, uint32_t* result, uint32_t grid,
                     const SplitTrace* trace)
{
    using namespace snappy_hip;
    std::vector<std::unique_ptr<GuardedCopy>> srcs;
    std::vector<std::unique_ptr<GuardedOut>> dsts;
    std::vector<RawItem> item_mem;
    for (uint32_t i = 0; i < count; ++i) {
        srcs.emplace_back(new GuardedCopy(src[i], (flags[i] & 1u) ? 0 : real_len[i]));
        dsts.emplace_back(new GuardedOut(capacity[i]));
        memset(dsts[i]->p, kDstFill, capacity[i]);
        item_mem.push_back(RawItem{(flags[i] & 1u) ? nullptr : srcs[i]->p, src_len[i], (flags[i] & 2u) ? nullptr : dsts[i]->p, capacity[i]});
    }
    if (item_mem.empty()) item_mem.push_back(RawItem{});
    if (max_segments > kSplitMaxWork) max_segments = kSplitMaxWork;
    if (max_units > kSplitMaxWork) max_units = kSplitMaxWork;
    const SplitLayout l = split_layout(count, max_segments, max_units);
    std::vector<uint8_t> scratch_mem(l.total + 512, kScratchJunk);      // never initialised on the GPU either
    uint8_t* scratch = scratch_mem.data() + (256 - ((uintptr_t)scratch_mem.data() & 255)) % 256;
    uint32_t* ctl = (uint32_t*)scratch;
    uint64_t* seg_prefix = (uint64_t*)(scratch + l.seg_prefix);
    uint64_t* unit_prefix = (uint64_t*)(scratch + l.unit_prefix);
    uint32_t* flag_words = (uint32_t*)(scratch + l.flags);
    uint64_t* table = (uint64_t*)(scratch + l.table);
    uint4* nodes = (uint4*)(scratch + l.nodes);
    uint32_t* cuts = (uint32_t*)(scratch + l.cuts);
    const RawItem* items = item_mem.data();
    emu::launch(1, 1024, [&] {
        raw_split_plan_kernel(items, count, unit_len, segment_bytes, max_segments, max_units, out_len, status, result, ctl, seg_prefix, unit_prefix,
                              flag_words, cuts);
    });
    if (trace) {                                                        // (steps 2-5 do not run when a limit is 0)
        memcpy(trace->plan_flags, flag_words, (size_t)count * sizeof(uint32_t));
        memcpy(trace->flags, flag_words, (size_t)count * sizeof(uint32_t));
        memset(trace->count, 0, 2 * (size_t)count * sizeof(uint32_t));
    }
    if (count && grid) {
        uint32_t counter = 0;
        if (max_segments && max_units) {
            emu::launch(grid, 64, [&] { raw_split_walk_kernel(items, count, segment_bytes, ctl, seg_prefix, flag_words, table, nodes, &counter); });
            emu::launch(count < 2 ? count : 2, 64, [&] {
                raw_split_resolve_kernel(items, count, unit_len, segment_bytes, out_len, seg_prefix, unit_prefix, flag_words, table, nodes, cuts);
            });
            counter = 0;
            emu::launch(grid, 64, [&] {
                raw_split_cuts_kernel(items, count, unit_len, ctl, out_len, seg_prefix, unit_prefix, flag_words, nodes, cuts, &counter);
            });
            if (trace) {
                memcpy(trace->flags, flag_words, (size_t)count * sizeof(uint32_t));
                uint64_t cut_at = 0, node_at = 0;
                for (uint32_t i = 0; i < count; ++i) {
                    trace->count[2 * i] = trace->count[2 * i + 1] = 0;
                    if ((trace->plan_flags[i] & (kSplitClassMask | kSplitFallback)) != kSplitSplit) continue;
                    const uint64_t n_cuts = unit_prefix[i + 1] - unit_prefix[i] + 1, n_nodes = seg_prefix[i + 1] - seg_prefix[i];
                    if (cut_at + n_cuts > trace->cut_room || node_at + 3 * n_nodes > trace->node_room) return -1;
                    memcpy(trace->cuts + cut_at, cuts + unit_prefix[i] + i, n_cuts * sizeof(uint32_t));
                    for (uint64_t s = 0; s < n_nodes; ++s) {
                        const uint4 node = nodes[seg_prefix[i] + s];
                        trace->nodes[node_at++] = node.x;
                        trace->nodes[node_at++] = node.y;
                        trace->nodes[node_at++] = node.z;
                    }
                    cut_at += n_cuts;
                    trace->count[2 * i] = (uint32_t)n_cuts;
                    trace->count[2 * i + 1] = (uint32_t)n_nodes;
                }
            }
            counter = 0;
            emu::launch(grid, 64, [&] { raw_split_units_kernel(items, count, unit_len, ctl, out_len, unit_prefix, flag_words, cuts, &counter); });
        }
        counter = 0;
        emu::launch(grid, 64, [&] { raw_split_serial_kernel(items, count, out_len, status, flag_words, result, &counter); });
    }
    int rc = 0;
    for (uint32_t k = 0; k < 256; ++k)
        if (scratch[l.total + k] != kScratchJunk) rc = kWroteBehindScratch;
    for (uint32_t i = 0; i < count; ++i) {
        if (!dsts[i]->intact()) rc = kWroteInFrontOfWindow;
        if (capacity[i]) memcpy(out[i], dsts[i]->p, capacity[i]);
    }
    return rc;
}

extern "C" {

int emu_raw_decompress_split(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity,
                             const uint32_t* flags, uint32_t count, uint32_t unit_len, uint32_t segment_bytes, uint64_t max_segments,
                             uint64_t max_units, uint8_t* const* out, uint64_t* out_len, uint32_t* status, uint32_t* result, uint32_t grid)
{
    return run_split(src, real_len, src_len, capacity, flags, count, unit_len, segment_bytes, max_segments, max_units, out, out_len, status, result,
                     grid, nullptr);
}

// The same call, and what its steps 1-4 left behind (SplitTrace).  -1: the trace's arrays are too small.
int emu_raw_decompress_split_traced(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity,
                                    const uint32_t* flags, uint32_t count, uint32_t unit_len, uint32_t segment_bytes, uint64_t max_segments,
                                    uint64_t max_units, uint8_t* const* out, uint64_t* out_len, uint32_t* status, uint32_t* result, uint32_t grid,
                                    uint32_t* plan_flags, uint32_t* step4_flags, uint32_t* trace_count, uint32_t* trace_cuts, uint64_t cut_room,
                                    uint32_t* trace_nodes, uint64_t node_room)
{
    const SplitTrace trace{plan_flags, step4_flags, trace_count, trace_cuts, cut_room, trace_nodes, node_room};
    return run_split(src, real_len, src_len, capacity, flags, count, unit_len, segment_bytes, max_segments, max_units, out, out_len, status, result,
                     grid, &trace);
}

}
