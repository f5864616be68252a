// The update kernels (pim-compression_amd/csrc/snappy_update.hpp) on the CPU wave emulator: a library of its own, built by
// tests/test_update_emulated.py.  Test infrastructure only.
#include "emu_runtime.cpp"
#include "snappy_update.hpp"

extern "C" {

// The five kernels as snappy_hip_update_ranges enqueues them, over one container (its stream copied to end at an
// inaccessible page: a read beyond it faults) and `write_count` writes whose src point into the caller's buffers.
// `grid` wavefronts recompress; form 3 = the stream form of K1's parse, 2 = the bulk form.  Returns 1 when the old stream
// is unchanged afterwards.
int emu_update_ranges(const uint8_t* stream, uint64_t stream_len, uint64_t* block_offsets, uint32_t desc_total_len, uint32_t desc_block_size,
                      uint32_t desc_num_blocks, uint32_t total_len, uint32_t block_size, const snappy_hip::WriteDesc* writes,
                      uint32_t write_count, uint32_t* write_status, uint8_t* new_stream, uint64_t capacity, uint64_t* new_offsets,
                      uint64_t* new_stream_len, uint32_t* result, uint32_t max_dirty, uint32_t grid, int form)
{
    using namespace snappy_hip;
    GuardedCopy old_stream(stream, stream_len);
    uint32_t unused[2] = {0, 0};
    const StreamDesc desc{old_stream.p, stream_len, block_offsets, unused, desc_total_len, desc_block_size, 0, desc_num_blocks};
    const uint32_t nb = (uint32_t)(((uint64_t)total_len + block_size - 1) / block_size);
    const uint32_t stride = (uint32_t)((4ull + 32ull + block_size + block_size / 6 + 15) & ~15ull);
    const UpdateLayout l = update_layout(block_size, nb, max_dirty, grid, stride);
    std::vector<uint8_t> scratch_mem(l.total + 256, 0xCD);              // never initialised on the GPU either ...
    uint8_t* scratch = scratch_mem.data() + (256 - ((uintptr_t)scratch_mem.data() & 255)) % 256;
    memset(scratch, 0, 256);                                            // ... but for the control line
    uint32_t* ctl = (uint32_t*)scratch;
    uint32_t* span = (uint32_t*)(scratch + l.span);
    uint32_t* rank = (uint32_t*)(scratch + l.rank);
    uint32_t* dirty = (uint32_t*)(scratch + l.dirty);
    uint32_t* dirty_bytes = (uint32_t*)(scratch + l.dirty_bytes);
    if (nb)
        emu::launch((nb + 255) / 256, 256, [&] {
            update_mark_kernel(&desc, total_len, block_size, nb, writes, write_count, ctl, span);
        });
    emu::launch(1, 1024, [&] {
        update_plan_kernel(&desc, total_len, block_size, nb, writes, write_count, write_status, max_dirty, ctl, span, rank, dirty,
                           new_stream_len, result);
    });
    uint32_t counter = 0;
    if (write_count && grid)
        emu::launch(grid, 64, [&] {
            if (form == 3)
                recompress_dirty_kernel<3>(&desc, total_len, block_size, writes, write_count, ctl, dirty, dirty_bytes, scratch + l.patch,
                                           l.patch_slot_bytes, scratch + l.cslots, stride, &counter);
            else
                recompress_dirty_kernel<2>(&desc, total_len, block_size, writes, write_count, ctl, dirty, dirty_bytes, scratch + l.patch,
                                           l.patch_slot_bytes, scratch + l.cslots, stride, &counter);
        });
    emu::launch(1, 1024, [&] {
        update_sizes_kernel(total_len, block_size, nb, ctl, span, rank, dirty_bytes, new_stream, capacity, new_offsets, new_stream_len, result);
    });
    if (nb)
        emu::launch(nb < 5 ? nb : 5, 256, [&] {
            merge_stream_kernel(&desc, nb, ctl, rank, scratch + l.cslots, stride, new_offsets, new_stream);
        });
    return memcmp(old_stream.p, stream, stream_len) == 0;
}

}
