// The range kernels (pim-compression_amd/csrc/snappy_ranges.hpp) on the CPU wave emulator: a library of its own, built by
// tests/test_ranges_emulated.py.  Test infrastructure only.
#include "emu_runtime.cpp"
#include "snappy_ranges.hpp"

extern "C" {

// range_pieces_kernel + decompress_ranges_kernel as snappy_hip_decompress_ranges enqueues them, over `count` containers
// (each stream copied to end at an inaccessible page: a read beyond it faults) and `range_count` ranges whose dst point
// into the caller's buffers.  `slots` scratch slots, `grid` wavefronts (at most `slots`).  Status per range in `status`.
void emu_decompress_ranges(uint32_t count, const uint8_t* const* streams, const uint64_t* stream_lens, uint64_t* const* block_offsets,
                           const uint32_t* total_lens, const uint32_t* block_sizes, const uint32_t* num_blocks,
                           const snappy_hip::RangeDesc* ranges, uint32_t range_count, uint32_t* status, uint32_t max_block_size,
                           uint32_t slots, uint32_t grid)
{
    std::vector<GuardedCopy*> copies;
    std::vector<snappy_hip::StreamDesc> descs(count + 1);
    uint32_t result[2] = {0, 0};
    for (uint32_t i = 0; i < count; ++i) {
        copies.push_back(new GuardedCopy(streams[i], stream_lens[i]));
        descs[i] = snappy_hip::StreamDesc{copies.back()->p, stream_lens[i], block_offsets[i], result, total_lens[i], block_sizes[i], 0,
                                          num_blocks[i]};
    }
    std::vector<uint64_t> prefix(snappy_hip::range_prefix_bytes(range_count) / 8, 0xdeadbeefdeadbeefull);   // never initialised on the GPU either
    const uint32_t slot_bytes = (uint32_t)snappy_hip::range_slot_bytes(max_block_size);
    std::vector<uint8_t> slot_mem((size_t)slots * slot_bytes + 64, 0xCD);
    for (uint32_t r = 0; r < range_count; ++r) status[r] = 0x77u;
    emu::launch(1, 1024, [&] {
        snappy_hip::range_pieces_kernel(descs.data(), count, ranges, range_count, status, max_block_size, prefix.data());
    });
    uint32_t counter = 0;
    const uint32_t g = grid < slots ? grid : slots;
    if (range_count && g)
        emu::launch(g, 64, [&] {
            snappy_hip::decompress_ranges_kernel(descs.data(), ranges, range_count, status, prefix.data(), slot_mem.data(), slot_bytes, &counter);
        });
    for (GuardedCopy* c : copies) delete c;
}

}
