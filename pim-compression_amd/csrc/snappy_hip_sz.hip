// snappy_hip_sz.hip -- the third source of libsnappy_hip.so: the Snappy framing format (.sz) and CRC-32C on the device
// (snappy_sz.hpp, snappy_crc32c.hpp; snappy_hip_sz_*_batch and snappy_hip_crc32c_batch, include/snappy_hip.h).
//
// As snappy_hip_raw_check_split.hip: the kernels of snappy_hip.hip are held, instruction for instruction, to what they were
// measured with, so a new feature's kernels live in a source of their own, which takes the __device__ pieces of the other
// headers without their kernels (SNAPPY_HIP_NO_KERNELS) and shares the host-side helpers through host_shared.hpp.
#define SNAPPY_HIP_NO_KERNELS
#undef SNAPPY_PROF          // (the probe builds' counters are snappy_hip.hip's own)
#undef SNAPPY_PAIR_PROBE
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "../../include/snappy_hip.h"
#include "host_shared.hpp"
#include "snappy_sz.hpp"

using namespace snappy_hip_host;

// SNAPPY_HIP_CRC_TABLES = 1 | 4: the table form of crc32c_wave (a 256-entry byte table, or slicing-by-4), for the comparison of
// DESIGN.md 3.12; anything else is the product's form (kCrcTables)
static int crc_tables()
{
    const char* v = getenv("SNAPPY_HIP_CRC_TABLES");
    const int t = (v && *v) ? atoi(v) : snappy_hip::kCrcTables;
    return (t == 1 || t == 4) ? t : snappy_hip::kCrcTables;
}

static bool chunk_len_ok(uint32_t chunk_len) { return chunk_len >= SNAPPY_HIP_MIN_BLOCK_SIZE && chunk_len <= SNAPPY_HIP_MAX_BLOCK_SIZE; }

extern "C" {

int snappy_hip_crc32c_batch(const snappy_hip_crc_item* d_items, uint32_t count, uint32_t* d_crc, void* stream)
{
    static_assert(sizeof(snappy_hip_crc_item) == sizeof(snappy_hip::CrcItem) && sizeof(snappy_hip::CrcItem) == 16, "snappy_hip_crc_item layout");
    if (count == 0) return SNAPPY_HIP_OK;
    if (!d_items || !d_crc) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    hipStream_t st = (hipStream_t)stream;
    return launch_counted(st, [&](uint32_t* counter) {
        const uint32_t grid = std::min(range_grid_cap(), count);
        const auto* items = reinterpret_cast<const snappy_hip::CrcItem*>(d_items);
        if (crc_tables() == 4) hipLaunchKernelGGL(snappy_hip::crc32c_batch_kernel<4>, dim3(grid), dim3(64), 0, st, items, count, d_crc, counter);
        else hipLaunchKernelGGL(snappy_hip::crc32c_batch_kernel<1>, dim3(grid), dim3(64), 0, st, items, count, d_crc, counter);
        return 0;
    });
}

uint64_t snappy_hip_sz_decompress_scratch_bytes(uint32_t count, uint32_t max_chunks) { return snappy_hip::sz_decode_layout(count, max_chunks).total; }

int snappy_hip_sz_decompress_batch(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t max_chunks, uint32_t flags, uint64_t* d_out_len,
                                   uint32_t* d_status, uint32_t* d_bad_chunk, uint32_t* d_result, void* d_scratch, uint64_t scratch_bytes,
                                   void* stream)
{
    using namespace snappy_hip;
    static_assert(sizeof(snappy_hip_raw_item) == sizeof(RawItem), "snappy_hip_raw_item layout");
    static_assert(SNAPPY_HIP_SZ_CRC_MISMATCH == kSzCrcMismatch && SNAPPY_HIP_SZ_UNSUPPORTED == kSzUnsupported && SNAPPY_HIP_SZ_NO_VERIFY == kSzNoVerify,
                  "sz status codes and flags");
    static_assert(sizeof(SzChunk) == 32, "SzChunk layout");
    if (flags & ~SNAPPY_HIP_SZ_NO_VERIFY) return fail(SNAPPY_HIP_ERR_ARG, "unknown flag (SNAPPY_HIP_SZ_NO_VERIFY is the only one)");
    if (!d_result || (count && (!d_items || !d_out_len || !d_status || !d_bad_chunk))) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    const SzDecodeLayout l = sz_decode_layout(count, max_chunks);
    if (scratch_bytes < l.total) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_sz_decompress_scratch_bytes)");
    hipStream_t st = (hipStream_t)stream;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    uint64_t* prefix = reinterpret_cast<uint64_t*>(scratch + l.prefix);
    SzChunk* chunks = reinterpret_cast<SzChunk*>(scratch + l.chunks);
    const auto* items = reinterpret_cast<const RawItem*>(d_items);
    const uint32_t item_grid = std::min(std::max(count, 1u), 4096u);
    if (count) hipLaunchKernelGGL(sz_index_kernel<false>, dim3(item_grid), dim3(64), 0, st, items, count, max_chunks, d_out_len, d_status, prefix, chunks);
    if (int rc = sz_enqueue_plan(st, count, max_chunks, d_status, d_result, d_scratch)) return rc;
    if (count == 0) return SNAPPY_HIP_OK;
    if (max_chunks) {
        hipLaunchKernelGGL(sz_index_kernel<true>, dim3(item_grid), dim3(64), 0, st, items, count, max_chunks, d_out_len, d_status, prefix, chunks);
        HIP_TRY(hipGetLastError());
    }
    return sz_enqueue_decode_finish(st, d_items, count, max_chunks, flags, d_status, d_bad_chunk, d_result, d_scratch);
}

}  // extern "C"

// (host_shared.hpp.  Defined here, behind the walks' launches, so that the templates are instantiated -- and the kernels emitted --
// in the order they always were: tools/kernel_asm_diff.py compares the text.)
namespace snappy_hip_host {

int sz_enqueue_plan(hipStream_t st, uint32_t count, uint32_t max_chunks, uint32_t* d_status, uint32_t* d_result, void* d_scratch)
{
    using namespace snappy_hip;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    const SzDecodeLayout l = sz_decode_layout(count, max_chunks);
    hipLaunchKernelGGL(sz_plan_kernel, dim3(1), dim3(1024), 0, st, count, max_chunks, d_status, d_result, reinterpret_cast<uint32_t*>(scratch),
                       reinterpret_cast<uint64_t*>(scratch + l.prefix));
    HIP_TRY(hipGetLastError());
    return 0;
}

int sz_enqueue_decode_finish(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t max_chunks, uint32_t flags,
                             uint32_t* d_status, uint32_t* d_bad_chunk, uint32_t* d_result, void* d_scratch)
{
    using namespace snappy_hip;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    const SzDecodeLayout l = sz_decode_layout(count, max_chunks);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(scratch);
    uint64_t* prefix = reinterpret_cast<uint64_t*>(scratch + l.prefix);
    SzChunk* chunks = reinterpret_cast<SzChunk*>(scratch + l.chunks);
    const auto* items = reinterpret_cast<const RawItem*>(d_items);
    if (max_chunks) {
        const int rc = launch_counted(st, [&](uint32_t* counter) {
            const uint32_t grid = std::min(range_grid_cap(), max_chunks);
            if (crc_tables() == 4) hipLaunchKernelGGL(sz_decode_chunks_kernel<4>, dim3(grid), dim3(64), 0, st, items, ctl, chunks, flags, counter);
            else hipLaunchKernelGGL(sz_decode_chunks_kernel<1>, dim3(grid), dim3(64), 0, st, items, ctl, chunks, flags, counter);
            return 0;
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(sz_finish_kernel, dim3(std::min(std::max(count, 1u), 4096u)), dim3(64), 0, st, count, prefix, chunks, d_status, d_bad_chunk,
                       d_result);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace snappy_hip_host

extern "C" {

uint64_t snappy_hip_sz_compress_bound(uint64_t src_len, uint32_t chunk_len)
{
    if (!chunk_len_ok(chunk_len)) return 0;
    return 10 + 8 * snappy_hip_num_blocks(src_len, chunk_len) + src_len;
}

uint64_t snappy_hip_sz_compress_scratch_bytes(uint32_t chunk_len, uint32_t count, uint32_t max_chunks)
{
    if (!chunk_len_ok(chunk_len)) return 0;
    return snappy_hip::sz_compress_layout(count, max_chunks, snappy_hip_slot_stride(chunk_len)).total;
}

int snappy_hip_sz_compress_batch(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks, uint64_t* d_out_len,
                                 uint32_t* d_status, uint32_t* d_result, void* d_scratch, uint64_t scratch_bytes, void* stream)
{
    if (int rc = sz_compress_check(d_items, count, chunk_len, max_chunks, d_out_len, d_status, d_result, d_scratch, scratch_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sz_compress_enqueue_plan(st, d_items, count, chunk_len, max_chunks, d_out_len, d_status, d_result, d_scratch)) return rc;
    if (count == 0) return SNAPPY_HIP_OK;
    if (max_chunks)
        if (int rc = sz_compress_enqueue_chunks(st, d_items, count, chunk_len, max_chunks, d_scratch)) return rc;
    return sz_compress_enqueue_crc_sizes_gather(st, d_items, count, chunk_len, max_chunks, d_out_len, d_status, d_result, d_scratch);
}

}  // extern "C"

// (host_shared.hpp: the steps of the call above, shared with snappy_hip_items_gt.hip)
namespace {
struct SzCompressParts {
    const snappy_hip::RawItem* items;
    uint32_t stride;
    snappy_hip::SzCompressLayout l;
    uint8_t* scratch;
    uint32_t* ctl;
    uint64_t* prefix;
    uint32_t* frag_bytes;
    uint64_t* place;
    uint32_t* crc;
    SzCompressParts(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks, void* d_scratch)
        : items(reinterpret_cast<const snappy_hip::RawItem*>(d_items)), stride(snappy_hip_slot_stride(chunk_len)),
          l(snappy_hip::sz_compress_layout(count, max_chunks, stride)), scratch(static_cast<uint8_t*>(d_scratch)), ctl(reinterpret_cast<uint32_t*>(scratch)),
          prefix(reinterpret_cast<uint64_t*>(scratch + l.prefix)), frag_bytes(reinterpret_cast<uint32_t*>(scratch + l.frag_bytes)),
          place(reinterpret_cast<uint64_t*>(scratch + l.place)), crc(reinterpret_cast<uint32_t*>(scratch + l.crc))
    {
    }
};
}  // namespace
namespace snappy_hip_host {

CompressParts sz_compress_parts(uint32_t count, uint32_t chunk_len, uint32_t max_chunks, void* d_scratch)
{
    const SzCompressParts p(nullptr, count, chunk_len, max_chunks, d_scratch);
    return CompressParts{p.ctl, p.prefix, p.frag_bytes, p.scratch + p.l.slots};
}

int sz_compress_check(const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks, const uint64_t* d_out_len,
                      const uint32_t* d_status, const uint32_t* d_result, const void* d_scratch, uint64_t scratch_bytes)
{
    if (!chunk_len_ok(chunk_len)) return fail(SNAPPY_HIP_ERR_ARG, "chunk_len must be 1..65535");
    if (!d_result || (count && (!d_items || !d_out_len || !d_status))) return fail(SNAPPY_HIP_ERR_ARG, "null device pointer");
    if (!d_scratch || ((uintptr_t)d_scratch & 255u)) return fail(SNAPPY_HIP_ERR_ARG, "d_scratch must be a 256-byte aligned device pointer");
    const snappy_hip::SzCompressLayout l = snappy_hip::sz_compress_layout(count, max_chunks, snappy_hip_slot_stride(chunk_len));
    if (scratch_bytes < l.total) return fail(SNAPPY_HIP_ERR_ARG, "scratch too small (snappy_hip_sz_compress_scratch_bytes)");
    return check_k1_knobs();
}

int sz_compress_enqueue_plan(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks,
                             uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch)
{
    const SzCompressParts p(d_items, count, chunk_len, max_chunks, d_scratch);
    hipLaunchKernelGGL(snappy_hip::sz_compress_plan_kernel, dim3(1), dim3(1024), 0, st, p.items, count, chunk_len, max_chunks, d_out_len, d_status,
                       d_result, p.ctl, p.prefix);
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}

int sz_compress_enqueue_chunks(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks,
                               void* d_scratch)
{
    using namespace snappy_hip;
    const SzCompressParts p(d_items, count, chunk_len, max_chunks, d_scratch);
    return launch_counted(st, [&](uint32_t* counter) {
        if (lds_table_stream_form(chunk_len)) {
            const uint32_t lds = lds_table_stream_lds_bytes(chunk_len);
            hipLaunchKernelGGL(sz_compress_chunks_kernel<3>, dim3(std::min(lds_table_resident_waves(lds), max_chunks)), dim3(64), lds, st, p.items,
                               count, chunk_len, p.ctl, p.prefix, p.frag_bytes, p.scratch + p.l.slots, p.stride, counter);
        } else {
            const uint32_t lds = lds_table_kernel_lds_bytes(chunk_len, true);
            hipLaunchKernelGGL(sz_compress_chunks_kernel<2>, dim3(std::min(lds_table_resident_waves(lds), max_chunks)), dim3(64), lds, st, p.items,
                               count, chunk_len, p.ctl, p.prefix, p.frag_bytes, p.scratch + p.l.slots, p.stride, counter);
        }
        return 0;
    });
}

int sz_compress_enqueue_crc_sizes_gather(hipStream_t st, const snappy_hip_raw_item* d_items, uint32_t count, uint32_t chunk_len, uint32_t max_chunks,
                                         uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_result, void* d_scratch)
{
    using namespace snappy_hip;
    const SzCompressParts p(d_items, count, chunk_len, max_chunks, d_scratch);
    if (count == 0) return SNAPPY_HIP_OK;
    if (max_chunks) {
        const int rc = launch_counted(st, [&](uint32_t* counter) {
            const uint32_t grid = std::min(range_grid_cap(), max_chunks);
            if (crc_tables() == 4) hipLaunchKernelGGL(sz_chunk_crc_kernel<4>, dim3(grid), dim3(64), 0, st, p.items, count, chunk_len, p.ctl, p.prefix, p.crc, counter);
            else hipLaunchKernelGGL(sz_chunk_crc_kernel<1>, dim3(grid), dim3(64), 0, st, p.items, count, chunk_len, p.ctl, p.prefix, p.crc, counter);
            return 0;
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(sz_sizes_kernel, dim3(std::min(count, 4096u)), dim3(64), 0, st, p.items, count, chunk_len, p.prefix, p.frag_bytes, p.place, d_out_len,
                       d_status, d_result);
    if (max_chunks)
        hipLaunchKernelGGL(sz_gather_kernel, dim3(std::min(max_chunks, 32768u)), dim3(256), 0, st, p.items, count, chunk_len, p.ctl, p.prefix, p.frag_bytes,
                           p.place, p.crc, p.scratch + p.l.slots, p.stride, d_status);
    HIP_TRY(hipGetLastError());
    return SNAPPY_HIP_OK;
}

}  // namespace snappy_hip_host
