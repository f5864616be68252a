// The raw-Snappy batch kernels (pim-compression_amd/csrc/snappy_raw.hpp) on the CPU wave emulator: a library of its own, built
// by tests/emu_raw_lib.py.  Test infrastructure only.
#include "emu_runtime.cpp"
#include "snappy_raw.hpp"

#include <memory>

namespace {

constexpr uint8_t kDstFill = 0xEE;           // what every dst holds before the kernels run

// Every item's src copied to end at an inaccessible page and every dst made a window of exactly `capacity` bytes between
// inaccessible pages, filled with kDstFill.  real_len: the bytes there are at src[i] (src_len[i] is what the item claims).
// flags bit 0: src is null; bit 1: dst is null.
struct GuardedItems {
    std::vector<std::unique_ptr<GuardedCopy>> srcs;
    std::vector<std::unique_ptr<GuardedOut>> dsts;
    std::vector<snappy_hip::RawItem> items;
    GuardedItems(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity, const uint32_t* flags, uint32_t count)
    {
        for (uint32_t i = 0; i < count; ++i) {
            srcs.emplace_back(new GuardedCopy(src[i], (flags[i] & 1u) ? 0 : real_len[i]));
            dsts.emplace_back(new GuardedOut(capacity[i]));
            memset(dsts[i]->p, kDstFill, capacity[i]);
            items.push_back(snappy_hip::RawItem{(flags[i] & 1u) ? nullptr : srcs[i]->p, src_len[i], (flags[i] & 2u) ? nullptr : dsts[i]->p,
                                                capacity[i]});
        }
        if (items.empty()) items.push_back(snappy_hip::RawItem{});
    }
    // copies every window out; returns 0, or kWroteInFrontOfWindow if a kernel wrote in front of one
    int collect(uint8_t* const* out, const uint64_t* capacity, uint32_t count) const
    {
        int rc = 0;
        for (uint32_t i = 0; i < count; ++i) {
            if (!dsts[i]->intact()) rc = kWroteInFrontOfWindow;
            if (capacity[i]) memcpy(out[i], dsts[i]->p, capacity[i]);
        }
        return rc;
    }
};

}  // namespace

extern "C" {

unsigned long long emu_raw_max_len() { return snappy_hip::kRawMaxLen; }
unsigned emu_raw_dst_fill() { return kDstFill; }

// raw_decompress_kernel over `count` items with `grid` wavefronts.  out[i]: capacity[i] bytes, the item's whole window
// afterwards.  A write behind a window (or a read behind a stream) faults: call from a child process.
int emu_raw_decompress(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity, const uint32_t* flags,
                       uint32_t count, uint8_t* const* out, uint64_t* out_len, uint32_t* status, uint32_t grid)
{
    GuardedItems g(src, real_len, src_len, capacity, flags, count);
    uint32_t counter = 0;
    if (count && grid)
        emu::launch(grid, 64, [&] { snappy_hip::raw_decompress_kernel(g.items.data(), count, out_len, status, &counter); });
    return g.collect(out, capacity, count);
}

// The four kernels as snappy_hip_raw_compress_batch enqueues them, `grid` wavefronts compressing; form 3 = the stream form of
// K1's parse, 2 = the bulk form.
int emu_raw_compress(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity, const uint32_t* flags,
                     uint32_t count, uint32_t block_size, uint32_t max_fragments, uint8_t* const* out, uint64_t* out_len, uint32_t* status, uint32_t* result,
                     uint32_t grid, int form)
{
    using namespace snappy_hip;
    GuardedItems g(src, real_len, src_len, capacity, flags, count);
    const uint32_t stride = (uint32_t)((4ull + 32ull + block_size + block_size / 6 + 15) & ~15ull);
    const RawLayout l = raw_layout(count, max_fragments, stride);
    std::vector<uint8_t> scratch_mem(l.total + 256, 0xCD);              // never initialised on the GPU either
    uint8_t* scratch = scratch_mem.data() + (256 - ((uintptr_t)scratch_mem.data() & 255)) % 256;
    uint32_t* ctl = (uint32_t*)scratch;
    uint64_t* prefix = (uint64_t*)(scratch + l.prefix);
    uint32_t* frag_bytes = (uint32_t*)(scratch + l.frag_bytes);
    uint64_t* place = (uint64_t*)(scratch + l.place);
    const RawItem* items = g.items.data();
    emu::launch(1, 1024, [&] { raw_plan_kernel(items, count, block_size, max_fragments, out_len, status, result, ctl, prefix); });
    uint32_t counter = 0;
    if (count && max_fragments && grid)
        emu::launch(grid, 64, [&] {
            if (form == 3) raw_compress_fragments_kernel<3>(items, count, block_size, ctl, prefix, frag_bytes, scratch + l.slots, stride, &counter);
            else raw_compress_fragments_kernel<2>(items, count, block_size, ctl, prefix, frag_bytes, scratch + l.slots, stride, &counter);
        });
    if (count) emu::launch(count < 3 ? count : 3, 64, [&] { raw_sizes_kernel(items, count, prefix, frag_bytes, place, out_len, status, result); });
    if (count && max_fragments)
        emu::launch(max_fragments < 5 ? max_fragments : 5, 256, [&] {
            raw_gather_kernel(items, count, ctl, prefix, frag_bytes, place, scratch + l.slots, stride, status);
        });
    return g.collect(out, capacity, count);
}

}
