// The split walk of .sz streams (pim-compression_amd/csrc/snappy_sz_split.hpp) on the CPU wave emulator, next to the base call's
// kernels (snappy_sz.hpp) in one library, built by tests/emu_sz_split_lib.py.  Test infrastructure only.
#include "emu_sz.cpp"          // GuardedItems, kDstFill and the base call's kernels
#include "snappy_sz_split.hpp"

namespace {

constexpr uint8_t kSplitScratchJunk = 0xCD;  // what the scratch, and the 256 bytes behind it, hold before the kernels run
constexpr int kWroteBehindSplitScratch = 101;

}  // namespace

extern "C" {

// segment_bytes != 0: the kernels as snappy_hip_sz_decompress_split_batch enqueues them, `grid` wavefronts in every launch over
// segments, items or chunks.  segment_bytes == 0: the kernels as snappy_hip_sz_decompress_batch enqueues them (result[2..3] are
// left alone).  Items as emu_sz_decompress.  chunk_words: the first min(ctl chunks, chunk_room) SzChunk records as the call left
// them, 8 words each; *chunk_count = ctl chunks.  path_on[i] / path_segs[i]: for an item the parallel walk proved, the segments
// on its path and all its segments; 0 otherwise.  Returns 0, 100 (a kernel wrote in front of a dst window) or 101 (behind the
// scratch); a read behind a stream or a write behind a window faults: call from a child process.
int emu_sz_split_decompress(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity,
                            const uint32_t* flags, uint32_t count, uint32_t max_chunks, uint32_t segment_bytes, uint64_t max_segments,
                            uint32_t call_flags, uint8_t* const* out, uint64_t* out_len, uint32_t* status, uint32_t* bad_chunk, uint32_t* result,
                            uint32_t grid, int tables, uint32_t* chunk_words, uint64_t chunk_room, uint32_t* chunk_count, uint32_t* path_on,
                            uint32_t* path_segs)
{
    using namespace snappy_hip;
    GuardedItems g(src, real_len, src_len, capacity, flags, count);
    if (max_segments > kSzSplitMaxSegments) max_segments = kSzSplitMaxSegments;
    const SzSplitLayout l = sz_split_layout(count, max_chunks, max_segments);
    std::vector<uint8_t> scratch_mem(l.total + 512, kSplitScratchJunk);     // never initialised on the GPU either
    uint8_t* scratch = scratch_mem.data() + (256 - ((uintptr_t)scratch_mem.data() & 255)) % 256;
    uint32_t* ctl = (uint32_t*)scratch;
    uint64_t* prefix = (uint64_t*)(scratch + l.d.prefix);
    SzChunk* chunks = (SzChunk*)(scratch + l.d.chunks);
    uint64_t* seg_prefix = (uint64_t*)(scratch + l.seg_prefix);
    uint32_t* item_flags = (uint32_t*)(scratch + l.flags);
    SzSeg* segs = (SzSeg*)(scratch + l.segs);
    const RawItem* items = g.items.data();
    const uint32_t item_grid = count < grid ? (count ? count : 1) : grid;
    const bool split = segment_bytes != 0;
    for (uint32_t i = 0; i < count; ++i) path_on[i] = path_segs[i] = 0;
    *chunk_count = 0;

    if (split) {
        emu::launch(1, 1024, [&] {
            sz_split_plan_kernel(items, count, segment_bytes, max_segments, out_len, status, result, ctl, prefix, seg_prefix, item_flags);
        });
        if (count) {
            if (max_segments) {
                emu::launch(grid, 64, [&] { sz_split_anchor_kernel(items, count, segment_bytes, ctl, seg_prefix, segs); });
                emu::launch(grid, 64, [&] { sz_split_walk_kernel(items, count, segment_bytes, ctl, seg_prefix, segs); });
            }
            emu::launch(item_grid, 64, [&] {
                sz_split_join_kernel(items, count, max_chunks, out_len, status, prefix, chunks, seg_prefix, item_flags, segs, result);
            });
        }
    } else if (count) {
        emu::launch(item_grid, 64, [&] { sz_index_kernel<false>(items, count, max_chunks, out_len, status, prefix, chunks); });
    }
    emu::launch(1, 1024, [&] { sz_plan_kernel(count, max_chunks, status, result, ctl, prefix); });
    if (count == 0) return 0;
    if (max_chunks) {
        if (split)
            emu::launch(grid, 64, [&] {
                sz_split_record_kernel(items, count, segment_bytes, ctl, status, prefix, chunks, seg_prefix, item_flags, segs);
            });
        else
            emu::launch(item_grid, 64, [&] { sz_index_kernel<true>(items, count, max_chunks, out_len, status, prefix, chunks); });
        uint32_t counter = 0;
        emu::launch(grid, 64, [&] {
            if (tables == 4) sz_decode_chunks_kernel<4>(items, ctl, chunks, call_flags, &counter);
            else sz_decode_chunks_kernel<1>(items, ctl, chunks, call_flags, &counter);
        });
    }
    emu::launch(item_grid, 64, [&] { sz_finish_kernel(count, prefix, chunks, status, bad_chunk, result); });

    *chunk_count = ctl[kSzCtlChunks];
    const uint64_t n_rec = *chunk_count < chunk_room ? *chunk_count : chunk_room;
    memcpy(chunk_words, chunks, n_rec * sizeof(SzChunk));
    if (split)
        for (uint32_t i = 0; i < count; ++i) {
            if (!(item_flags[i] & kSzItemProven)) continue;
            path_segs[i] = (uint32_t)(seg_prefix[i + 1] - seg_prefix[i]);
            for (uint64_t p = seg_prefix[i]; p < seg_prefix[i + 1]; ++p) path_on[i] += segs[p].on_path ? 1u : 0u;
        }
    for (uint32_t k = 0; k < 256; ++k)
        if (scratch[l.total + k] != kSplitScratchJunk) return kWroteBehindSplitScratch;
    return g.collect(out, capacity, count);
}

}
