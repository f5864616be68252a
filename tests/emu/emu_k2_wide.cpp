// The wide block decoder (pim-compression_amd/csrc/snappy_k2_wide.hpp) on the CPU wave emulator: a library of its own, built
// by tests/emu_k2_wide_lib.py.  Test infrastructure only.
#include "emu_runtime.cpp"
#include "snappy_k2_wide.hpp"

extern "C" {

// k2_wide_kernel as snappy_hip_decompress_blocks_wide launches it: `grid` workgroups of waves_per_block wavefronts over the
// blocks of one container (offsets: one u64 per block).  The stream ends at an inaccessible page, the output is a window of
// exactly total_len bytes between inaccessible pages (copied to out_user afterwards); status: one word per block; result: the
// four result words.  Returns 0, or 100 if the kernel wrote in front of the window; a write behind it or a read behind the
// stream faults: call from a child process.
int emu_k2_wide(const uint8_t* stream_in, uint64_t stream_len, const uint64_t* offsets, uint64_t total_len, uint32_t block_size,
                uint32_t waves_per_block, uint32_t grid, uint8_t* out_user, uint32_t* status, uint32_t* result)
{
    result[0] = result[1] = result[2] = result[3] = 0;
    if (total_len == 0 || block_size == 0) return 0;
    const uint32_t nb = (uint32_t)((total_len + block_size - 1) / block_size);
    GuardedCopy guarded(stream_in, stream_len);
    GuardedOut guarded_out(total_len);
    uint32_t counter = 0;
    emu::launch(grid < nb ? grid : nb, 64 * waves_per_block, [&] {
        snappy_hip::k2_wide_kernel(guarded.p, stream_len, offsets, total_len, block_size, guarded_out.p, status, nb, result, &counter);
    });
    if (!guarded_out.intact()) return kWroteInFrontOfWindow;
    memcpy(out_user, guarded_out.p, total_len);
    return 0;
}

unsigned emu_k2_wide_max_csz() { return snappy_hip::kWideMaxCsz; }
unsigned emu_k2_wide_lds_bytes() { return snappy_hip::kWideLdsBytes; }
}
