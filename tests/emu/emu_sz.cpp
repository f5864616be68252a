// The .sz kernels (pim-compression_amd/csrc/snappy_sz.hpp, snappy_crc32c.hpp) on the CPU wave emulator: a library of its own,
// built by tests/emu_sz_lib.py.  Test infrastructure only.
#include "emu_runtime.cpp"
#include "snappy_sz.hpp"

#include <memory>

namespace {

constexpr uint8_t kDstFill = 0xEE;           // what every dst holds before the kernels run

// As tests/emu/emu_raw.cpp: every item's src copied to end at an inaccessible page and every dst made a window of exactly
// `capacity` bytes between inaccessible pages, filled with kDstFill.  flags bit 0: src is null; bit 1: dst is null.
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

}  // namespace

extern "C" {

unsigned emu_sz_dst_fill() { return kDstFill; }
unsigned emu_sz_crc_mask(unsigned c) { return snappy_hip::crc_mask(c); }

// crc32c_batch_kernel<tables> over `count` items with `grid` wavefronts.  Item i's len[i] bytes are followed by pad[i] bytes
// of another value before the inaccessible page: pad 0 = a read of one byte beyond the item faults; the pads move the item's
// first byte over every alignment.
int emu_crc32c_batch(const uint8_t* const* src, const uint64_t* len, const uint32_t* pad, uint32_t count, uint32_t* crc, uint32_t grid, int tables)
{
    std::vector<std::unique_ptr<GuardedCopy>> copies;
    std::vector<snappy_hip::CrcItem> items;
    for (uint32_t i = 0; i < count; ++i) {
        std::vector<uint8_t> padded(src[i], src[i] + len[i]);
        padded.resize(len[i] + pad[i], 0x5C);
        copies.emplace_back(new GuardedCopy(padded.data(), padded.size()));
        items.push_back(snappy_hip::CrcItem{copies[i]->p, len[i]});
    }
    uint32_t counter = 0;
    if (count && grid)
        emu::launch(grid, 64, [&] {
            if (tables == 4) snappy_hip::crc32c_batch_kernel<4>(items.data(), count, crc, &counter);
            else snappy_hip::crc32c_batch_kernel<1>(items.data(), count, crc, &counter);
        });
    return 0;
}

// gf_mul and x_pow_words, for the model's comparison
unsigned emu_gf_mul(unsigned a, unsigned b) { return snappy_hip::gf_mul(a, b); }
unsigned emu_x_pow_words(unsigned words) { return snappy_hip::x_pow_words(words); }

// The kernels as snappy_hip_sz_decompress_batch enqueues them, `grid` wavefronts decoding.
int emu_sz_decompress(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity, const uint32_t* flags,
                      uint32_t count, uint32_t max_chunks, uint32_t call_flags, uint8_t* const* out, uint64_t* out_len, uint32_t* status,
                      uint32_t* bad_chunk, uint32_t* result, uint32_t grid, int tables)
{
    using namespace snappy_hip;
    GuardedItems g(src, real_len, src_len, capacity, flags, count);
    const SzDecodeLayout l = sz_decode_layout(count, max_chunks);
    Scratch scratch(l.total);
    uint32_t* ctl = (uint32_t*)scratch.p;
    uint64_t* prefix = (uint64_t*)(scratch.p + l.prefix);
    SzChunk* chunks = (SzChunk*)(scratch.p + l.chunks);
    const RawItem* items = g.items.data();
    const uint32_t item_grid = count < 3 ? (count ? count : 1) : 3;
    if (count) emu::launch(item_grid, 64, [&] { sz_index_kernel<false>(items, count, max_chunks, out_len, status, prefix, chunks); });
    emu::launch(1, 1024, [&] { sz_plan_kernel(count, max_chunks, status, result, ctl, prefix); });
    if (count == 0) return 0;
    if (max_chunks) {
        emu::launch(item_grid, 64, [&] { sz_index_kernel<true>(items, count, max_chunks, out_len, status, prefix, chunks); });
        uint32_t counter = 0;
        emu::launch(grid, 64, [&] {
            if (tables == 4) sz_decode_chunks_kernel<4>(items, ctl, chunks, call_flags, &counter);
            else sz_decode_chunks_kernel<1>(items, ctl, chunks, call_flags, &counter);
        });
    }
    emu::launch(item_grid, 64, [&] { sz_finish_kernel(count, prefix, chunks, status, bad_chunk, result); });
    return g.collect(out, capacity, count);
}

// The kernels as snappy_hip_sz_compress_batch enqueues them; form 3 = the stream form of K1's parse, 2 = the bulk form.
int emu_sz_compress(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint64_t* capacity, const uint32_t* flags,
                    uint32_t count, uint32_t chunk_len, uint32_t max_chunks, uint8_t* const* out, uint64_t* out_len, uint32_t* status, uint32_t* result,
                    uint32_t grid, int form, int tables)
{
    using namespace snappy_hip;
    GuardedItems g(src, real_len, src_len, capacity, flags, count);
    const uint32_t stride = (uint32_t)((4ull + 32ull + chunk_len + chunk_len / 6 + 15) & ~15ull);
    const SzCompressLayout l = sz_compress_layout(count, max_chunks, stride);
    Scratch scratch(l.total);
    uint32_t* ctl = (uint32_t*)scratch.p;
    uint64_t* prefix = (uint64_t*)(scratch.p + l.prefix);
    uint32_t* frag_bytes = (uint32_t*)(scratch.p + l.frag_bytes);
    uint64_t* place = (uint64_t*)(scratch.p + l.place);
    uint32_t* crc = (uint32_t*)(scratch.p + l.crc);
    const RawItem* items = g.items.data();
    emu::launch(1, 1024, [&] { sz_compress_plan_kernel(items, count, chunk_len, max_chunks, out_len, status, result, ctl, prefix); });
    if (count == 0) return 0;
    if (max_chunks && grid) {
        uint32_t counter = 0;
        emu::launch(grid, 64, [&] {
            if (form == 3) sz_compress_chunks_kernel<3>(items, count, chunk_len, ctl, prefix, frag_bytes, scratch.p + l.slots, stride, &counter);
            else sz_compress_chunks_kernel<2>(items, count, chunk_len, ctl, prefix, frag_bytes, scratch.p + l.slots, stride, &counter);
        });
        counter = 0;
        emu::launch(grid, 64, [&] {
            if (tables == 4) sz_chunk_crc_kernel<4>(items, count, chunk_len, ctl, prefix, crc, &counter);
            else sz_chunk_crc_kernel<1>(items, count, chunk_len, ctl, prefix, crc, &counter);
        });
    }
    emu::launch(count < 3 ? count : 3, 64, [&] { sz_sizes_kernel(items, count, chunk_len, prefix, frag_bytes, place, out_len, status, result); });
    if (max_chunks)
        emu::launch(max_chunks < 5 ? max_chunks : 5, 256, [&] {
            sz_gather_kernel(items, count, chunk_len, ctl, prefix, frag_bytes, place, crc, scratch.p + l.slots, stride, status);
        });
    return g.collect(out, capacity, count);
}

}
