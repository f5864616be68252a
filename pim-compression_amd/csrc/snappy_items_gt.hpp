// snappy_items_gt.hpp -- the fragments of a raw batch, or the chunks of a .sz batch, compressed by K1's GLOBAL-table wavefronts
// (snappy_hip_raw_compress_batch_tables, snappy_hip_sz_compress_batch_tables, include/snappy_hip.h).
//
// The base calls parse every fragment with K1's LDS-table form (raw_compress_fragments_kernel, sz_compress_chunks_kernel): at
// 32 KiB fragments the LDS holds about four such wavefronts per CU.  The container's compressor keeps its table in global
// memory behind a filter (and, for full-size tables, a slot cache) in LDS, and fills the CU's wavefront slots.  The one kernel
// here is that compressor's table set-up (compress_blocks_global_table_kernel, snappy_kernels.hpp) around the raw kernel's trip
// (item and fragment from the prefix, slot f, frag_bytes + f): the same parse -- compress_one_block_stream /
// compress_one_block_bulk, unchanged -- on the same bytes, so slot f and frag_bytes[f] are what the LDS-table form leaves and
// everything behind this kernel (sizes, CRCs, gather) is the base call's.
//
// A fragment never sees what another left in its wavefront's table: the parse clears the `written` filter (and the slot
// cache) at the start of every block, and a slot that was not written in this block is answered from a register.  So the
// tables need no initialisation, whichever item the wavefront's last fragment belonged to.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_kernels.hpp"   // FilteredGlobalTable, CachedGlobalTable, compress_one_block_stream, compress_one_block_bulk
#include "snappy_raw.hpp"       // RawItem, kRawCtlFragments

namespace snappy_hip {

// bytes of one wavefront's table in the workspace, whichever kind the block size selects (u32 entries behind the filter alone,
// u16 positions behind the slot cache): the stride snappy_hip_compress_blocks uses
constexpr uint64_t kItemsGtTableBytes = (uint64_t)kMaxTableEntries * sizeof(uint32_t);
constexpr uint32_t kItemsGtResultWord = 2;   // d_result[2]: fragments compressed by global-table wavefronts

// kForm: the form of K1's parse (3 = stream, 2 = bulk); kCacheSlots: 512 = the slot cache in front of the table (blocks with
// full-size tables), 0 = the filter alone.  ctl[0] is the number of fragments (kRawCtlFragments, kSzCtlChunks); wavefront w's
// table is table_scratch + w * kMaxTableEntries words.
template <int kForm, uint32_t kCacheSlots>
__global__ __launch_bounds__(64) void item_fragments_global_table_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t block_size,
                                                                         const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ prefix,
                                                                         uint32_t* __restrict__ frag_bytes, uint8_t* __restrict__ slots,
                                                                         uint32_t slot_stride, uint32_t* table_scratch, uint32_t* __restrict__ result,
                                                                         uint32_t* next_fragment)
{
    static_assert(kForm == 2 || kForm == 3, "the bulk (2) and the stream (3) form of the parse exist");
    static_assert(kCacheSlots == 0 || kCacheSlots == 512, "the slot cache has 512 slots or is off");
    __shared__ __attribute__((aligned(16))) uint8_t dup_scratch[kForm == 3 ? stream_scratch_bytes(kStreamSlotsGlobal) : kDupSlots];
    __shared__ __attribute__((aligned(16))) uint32_t slot_state[kMaxTableEntries / 32];   // the "slot written in this block" filter
    __shared__ __attribute__((aligned(16))) uint32_t slot_cache[kCacheSlots ? kCacheSlots : 4];
    const uint32_t lane = threadIdx.x;
    using Table = typename std::conditional<kCacheSlots != 0, CachedGlobalTable<(kCacheSlots ? kCacheSlots : 1024u)>, FilteredGlobalTable>::type;
    Table table;
    if constexpr (kCacheSlots != 0) {
        table.t = (uint16_t*)table_scratch + (size_t)blockIdx.x * kMaxTableEntries;
        table.written = (lds_words_t)slot_state;
        table.cache = (lds_words_t)slot_cache;
    } else {
        table.t = table_scratch + (size_t)blockIdx.x * kMaxTableEntries;
        table.written = (lds_words_t)slot_state;
        table.empty = 0;
    }
    const uint32_t fragments = uni(ctl[kRawCtlFragments]);
    uint32_t taken = 0;

    for (;;) {
        const uint32_t f = draw_work(next_fragment, lane);
        if (f >= fragments) break;
        const uint32_t i = prefix_owner<false>(prefix, count, f);
        const uint8_t* src = load_global_ptr(&items[i].src);
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));   // (validated: < 4 GiB)
        const uint64_t start = (f - uld64(reinterpret_cast<const uint8_t*>(prefix + i))) * block_size;
        const uint64_t left = src_len - start;
        const uint32_t n = left < block_size ? (uint32_t)left : block_size;
        uint8_t* out = slots + (uint64_t)f * slot_stride;
        if constexpr (kForm == 3) {
            SoloMate solo;
            compress_one_block_stream<Table, kStreamSlotsGlobal>(src, start, src_len, n, out, table, lane, frag_bytes + f, (lds_bytes_t)dup_scratch, solo);
        } else {
            compress_one_block_bulk<Table, 64>(src, start, src_len, n, out, table, lane, frag_bytes + f, (lds_bytes_t)dup_scratch);
        }
        ++taken;
        __syncthreads();
    }
    if (lane == 0 && taken) atomicAdd(result + kItemsGtResultWord, taken);
}

}  // namespace snappy_hip
