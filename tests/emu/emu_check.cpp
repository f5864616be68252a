// The check kernels (pim-compression_amd/csrc/snappy_check.hpp) on the CPU wave emulator: a library of its own, built by
// tests/emu_check_lib.py.  Test infrastructure only.
#include "emu_runtime.cpp"

// single-threaded fibers: a plain read-modify-write is atomic (as atomicAdd / atomicOr in hip/hip_runtime.h)
static inline uint32_t atomicMin(uint32_t* p, uint32_t v)
{
    const uint32_t old = *p;
    if (v < old) *p = v;
    return old;
}

#include "snappy_check.hpp"

#include <memory>

namespace {

constexpr uint32_t kResultJunk = 0xABABABABu;   // what the result words and their guards hold before the kernels run
constexpr uint32_t kStatusJunk = 0x77777777u;   // ... and the per-block status arrays and theirs

std::vector<uint8_t> junk_scratch(uint64_t bytes, uint8_t** aligned)
{
    std::vector<uint8_t> mem(bytes + 256, 0xCD);                       // never initialised on the GPU either
    *aligned = mem.data() + (256 - ((uintptr_t)mem.data() & 255)) % 256;
    return mem;
}

}  // namespace

extern "C" {

unsigned emu_check_result_junk() { return kResultJunk; }
unsigned emu_check_status_junk() { return kStatusJunk; }

// check_plan_kernel + check_kernel over `count` containers with `grid` wavefronts.  Every stream is copied to end at an
// inaccessible page (real_len[i] bytes are there; stream_len[i] is what the descriptor claims).  flags bit 0: the descriptor's
// stream is null; bit 1: its block_offsets are null.  status_mode 0: no status array at all; 1: an array of null pointers;
// 2: a status array of status_words[i] words for every container, copied to status_out + status_at[i] afterwards.
// results_out: 4 * count words.  Returns 0, or bit 0 set when a word beside the results was written, bit 1 when a word beside
// a status array was.  A read behind a stream faults: call from a child process.
int emu_check_blocks(const uint8_t* const* stream, const uint64_t* real_len, const uint64_t* stream_len, const uint64_t* const* offsets,
                     const uint32_t* total_len, const uint32_t* block_size, const uint32_t* num_blocks, const uint32_t* flags, uint32_t count,
                     int status_mode, const uint32_t* status_words, const uint64_t* status_at, uint32_t* status_out, uint32_t* results_out,
                     uint32_t grid)
{
    using namespace snappy_hip;
    std::vector<std::unique_ptr<GuardedCopy>> copies;
    std::vector<StreamDesc> descs;
    std::vector<std::vector<uint32_t>> status;
    std::vector<uint32_t*> status_ptr;
    for (uint32_t i = 0; i < count; ++i) {
        copies.emplace_back(new GuardedCopy(stream[i], real_len[i]));
        descs.push_back(StreamDesc{(flags[i] & 1u) ? nullptr : copies[i]->p, stream_len[i], (flags[i] & 2u) ? nullptr : const_cast<uint64_t*>(offsets[i]),
                                   nullptr, total_len[i], block_size[i], 0, num_blocks[i]});
        status.emplace_back((size_t)status_words[i] + 2, kStatusJunk);
        status_ptr.push_back(status_mode == 2 ? status[i].data() + 1 : nullptr);
    }
    if (descs.empty()) descs.push_back(StreamDesc{});
    if (status_ptr.empty()) status_ptr.push_back(nullptr);
    std::vector<uint32_t> results(4 * (size_t)count + 2, kResultJunk);
    uint8_t* scratch;
    const std::vector<uint8_t> scratch_mem = junk_scratch(check_prefix_bytes(count), &scratch);
    uint64_t* prefix = (uint64_t*)scratch;
    emu::launch(1, 1024, [&] { check_plan_kernel(descs.data(), count, results.data() + 1, prefix); });
    uint32_t counter = 0;
    if (grid)
        emu::launch(grid, 64, [&] { check_kernel(descs.data(), count, status_mode ? status_ptr.data() : nullptr, results.data() + 1, prefix, &counter); });
    int rc = 0;
    if (results.front() != kResultJunk || results.back() != kResultJunk) rc |= 1;
    memcpy(results_out, results.data() + 1, 4 * (size_t)count * sizeof(uint32_t));
    for (uint32_t i = 0; i < count; ++i) {
        if (status[i].front() != kStatusJunk || status[i].back() != kStatusJunk) rc |= 2;
        if (status_words[i]) memcpy(status_out + status_at[i], status[i].data() + 1, (size_t)status_words[i] * sizeof(uint32_t));
    }
    return rc;
}

// ONE block checked alone, as a container of one block of out_len bytes whose size word is at stream + at: the twin of
// emu_decompress_block.  Returns the block's status, or 100 + the container's first result word when the result words
// disagree with it.
int emu_check_block(const uint8_t* stream_in, uint64_t stream_len, uint64_t at, uint32_t out_len)
{
    using namespace snappy_hip;
    if (out_len == 0) return 1;
    GuardedCopy guarded(stream_in, stream_len);
    uint64_t boff = at;
    uint32_t status = 9, counter = 0;
    uint32_t* status_ptr = &status;
    uint32_t results[4] = {kResultJunk, kResultJunk, kResultJunk, kResultJunk};
    StreamDesc d{guarded.p, stream_len, &boff, nullptr, out_len, out_len, 0, 1};
    uint8_t* scratch;
    const std::vector<uint8_t> scratch_mem = junk_scratch(check_prefix_bytes(1), &scratch);
    uint64_t* prefix = (uint64_t*)scratch;
    emu::launch(1, 1024, [&] { check_plan_kernel(&d, 1, results, prefix); });
    emu::launch(1, 64, [&] { check_kernel(&d, 1, &status_ptr, results, prefix, &counter); });
    const bool agree = status == kBlockOk ? (results[0] == kBlockOk && results[1] == 0 && results[2] == kCheckNone && results[3] == 0)
                                          : (status == kBlockInvalid && results[0] == kBlockInvalid && results[1] == 1 && results[2] == 0 && results[3] == 0);
    return agree ? (int)status : 100 + (int)results[0];
}

// raw_check_kernel over `count` items with `grid` wavefronts; every src ends at an inaccessible page.  flags bit 0: src is
// null.  dst is a pointer that must not be followed and dst_capacity is 0: both are ignored.
void emu_raw_check(const uint8_t* const* src, const uint64_t* real_len, const uint64_t* src_len, const uint32_t* flags, uint32_t count,
                   uint64_t* out_len, uint32_t* status, uint32_t grid)
{
    using namespace snappy_hip;
    std::vector<std::unique_ptr<GuardedCopy>> srcs;
    std::vector<RawItem> items;
    for (uint32_t i = 0; i < count; ++i) {
        srcs.emplace_back(new GuardedCopy(src[i], (flags[i] & 1u) ? 0 : real_len[i]));
        items.push_back(RawItem{(flags[i] & 1u) ? nullptr : srcs[i]->p, src_len[i], (uint8_t*)(uintptr_t)16, 0});
    }
    if (items.empty()) items.push_back(RawItem{});
    uint32_t counter = 0;
    if (count && grid) emu::launch(grid, 64, [&] { raw_check_kernel(items.data(), count, out_len, status, &counter); });
}

}
