// The raw / .sz compress calls with K1's global-table wavefronts (pim-compression_amd/csrc/snappy_items_gt.hpp) on the CPU wave
// emulator: a library of its own, built by tests/emu_items_gt_lib.py.  Test infrastructure only.
#include "emu_runtime.cpp"
#include "snappy_sz.hpp"
#include "snappy_items_gt.hpp"

#include <memory>

namespace {

constexpr uint8_t kDstFill = 0xEE;           // what every dst holds before the kernels run

// As tests/emu/emu_raw.cpp: every item's src copied to end at an inaccessible page and every dst made a window of exactly
// `capacity` bytes between inaccessible pages, filled with kDstFill.  flags bit 0: src is null; bit 1: dst is null.
struct GuardedItems {
    std::vector<std::unique_ptr<GuardedCopy>> srcs;
    std::vector<std::unique_ptr<GuardedOut>> dsts;
    std::vector<snappy_hip::RawItem> items;
    GuardedItems(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity, const uint32_t* flags,
                 const uint32_t* spare, uint32_t count)
    {
        for (uint32_t i = 0; i < count; ++i) {
            // spare[i] bytes in front of the source: its first byte at every alignment
            std::vector<uint8_t> shifted(spare[i], 0xA7);
            if (!(flags[i] & 1u)) shifted.insert(shifted.end(), src[i], src[i] + real_len[i]);
            srcs.emplace_back(new GuardedCopy(shifted.data(), (flags[i] & 1u) ? 0 : shifted.size()));
            dsts.emplace_back(new GuardedOut(capacity[i]));
            memset(dsts[i]->p, kDstFill, capacity[i]);
            items.push_back(snappy_hip::RawItem{(flags[i] & 1u) ? nullptr : srcs[i]->p + spare[i], src_len[i], (flags[i] & 2u) ? nullptr : dsts[i]->p,
                                                capacity[i]});
        }
        if (items.empty()) items.push_back(snappy_hip::RawItem{});
    }
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

struct Scratch {
    std::vector<uint8_t> mem;
    uint8_t* p;
    explicit Scratch(uint64_t bytes) : mem(bytes + 256, 0xCD)            // never initialised on the GPU either
    {
        p = mem.data() + (256 - ((uintptr_t)mem.data() & 255)) % 256;
    }
};

template <class... A>
void launch_items_gt(uint32_t grid, int form, int cached, A... a)
{
    using namespace snappy_hip;
    emu::launch(grid, 64, [&] {
        if (form == 3 && cached) item_fragments_global_table_kernel<3, 512>(a...);
        else if (cached) item_fragments_global_table_kernel<2, 512>(a...);
        else if (form == 3) item_fragments_global_table_kernel<3, 0>(a...);
        else item_fragments_global_table_kernel<2, 0>(a...);
    });
}

}  // namespace

extern "C" {

unsigned emu_items_gt_dst_fill() { return kDstFill; }
unsigned long long emu_items_gt_table_bytes() { return snappy_hip::kItemsGtTableBytes; }

// The kernels as snappy_hip_raw_compress_batch_tables (sz == 0) or snappy_hip_sz_compress_batch_tables (sz != 0) enqueues them
// when it takes the global-table kernel: `grid` wavefronts compressing, form 3 = the stream form of K1's parse, 2 = the bulk
// form; cached != 0 = the slot cache in front of the table.  tables: grid tables of emu_items_gt_table_bytes(), the caller's, in
// whatever state they are.  result: four words.
int emu_items_gt_compress(int sz, const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity,
                          const uint32_t* flags, const uint32_t* spare, uint32_t count, uint32_t block_size, uint32_t max_units, uint8_t* const* out,
                          uint64_t* out_len, uint32_t* status, uint32_t* result, uint32_t grid, int form, int cached, uint32_t* tables)
{
    using namespace snappy_hip;
    GuardedItems g(src, real_len, src_len, capacity, flags, spare, count);
    const uint32_t stride = (uint32_t)((4ull + 32ull + block_size + block_size / 6 + 15) & ~15ull);
    const RawItem* items = g.items.data();
    result[2] = result[3] = 0;                                           // (the call's memset)
    uint32_t counter = 0;
    if (!sz) {
        const RawLayout l = raw_layout(count, max_units, stride);
        Scratch scratch(l.total);
        uint32_t* ctl = (uint32_t*)scratch.p;
        uint64_t* prefix = (uint64_t*)(scratch.p + l.prefix);
        uint32_t* frag_bytes = (uint32_t*)(scratch.p + l.frag_bytes);
        uint64_t* place = (uint64_t*)(scratch.p + l.place);
        emu::launch(1, 1024, [&] { raw_plan_kernel(items, count, block_size, max_units, out_len, status, result, ctl, prefix); });
        if (count && max_units && grid)
            launch_items_gt(grid, form, cached, items, count, block_size, (const uint32_t*)ctl, (const uint64_t*)prefix, frag_bytes, scratch.p + l.slots,
                            stride, tables, result, &counter);
        if (count) emu::launch(count < 3 ? count : 3, 64, [&] { raw_sizes_kernel(items, count, prefix, frag_bytes, place, out_len, status, result); });
        if (count && max_units)
            emu::launch(max_units < 5 ? max_units : 5, 256, [&] {
                raw_gather_kernel(items, count, ctl, prefix, frag_bytes, place, scratch.p + l.slots, stride, status);
            });
        return g.collect(out, capacity, count);
    }
    const SzCompressLayout l = sz_compress_layout(count, max_units, stride);
    Scratch scratch(l.total);
    uint32_t* ctl = (uint32_t*)scratch.p;
    uint64_t* prefix = (uint64_t*)(scratch.p + l.prefix);
    uint32_t* frag_bytes = (uint32_t*)(scratch.p + l.frag_bytes);
    uint64_t* place = (uint64_t*)(scratch.p + l.place);
    uint32_t* crc = (uint32_t*)(scratch.p + l.crc);
    emu::launch(1, 1024, [&] { sz_compress_plan_kernel(items, count, block_size, max_units, out_len, status, result, ctl, prefix); });
    if (count == 0) return 0;
    if (max_units && grid) {
        launch_items_gt(grid, form, cached, items, count, block_size, (const uint32_t*)ctl, (const uint64_t*)prefix, frag_bytes, scratch.p + l.slots, stride,
                        tables, result, &counter);
        counter = 0;
        emu::launch(grid, 64, [&] { sz_chunk_crc_kernel<1>(items, count, block_size, ctl, prefix, crc, &counter); });
    }
    emu::launch(count < 3 ? count : 3, 64, [&] { sz_sizes_kernel(items, count, block_size, prefix, frag_bytes, place, out_len, status, result); });
    if (max_units)
        emu::launch(max_units < 5 ? max_units : 5, 256, [&] {
            sz_gather_kernel(items, count, block_size, ctl, prefix, frag_bytes, place, crc, scratch.p + l.slots, stride, status);
        });
    return g.collect(out, capacity, count);
}

}
