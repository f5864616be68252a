// snappy_ranges.hpp -- byte ranges of block-framed containers, decoded without the rest of them
// (snappy_hip_decompress_ranges, include/snappy_hip.h).
//
// The blocks of the format are independent, so bytes [offset, offset + length) of a container need only the blocks they
// touch.  The work unit is a PIECE: a pair (range r, block b) for every block b that range r touches.  Two kernels:
//   * range_pieces_kernel (one workgroup, the planner loop of scan_block_bytes_kernel): validates every range, initialises its
//     status and writes the exclusive prefix of the ranges' piece counts;
//   * decompress_ranges_kernel (persistent wavefronts, one counter, as K2): a wavefront draws a piece index, finds its range
//     by a binary search over the prefix and decodes the block with K2's own decoder (k2_decode_block).  A block wholly
//     inside the range is decoded in place, at dst_r + (b * block_size - offset_r); the first and last block of a range,
//     when only part of them is wanted, are decoded into the wavefront's own scratch slot and the wanted bytes copied out.
// Strict as K2: every touched block is decoded in full, and a range is OK iff every block it touches is.  Nothing outside
// [dst_r, dst_r + length_r) is written (the slots excepted), whatever the stream holds.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_kernels.hpp"

namespace snappy_hip {

constexpr uint64_t kMaxRangePieces = 1ull << 31;    // pieces one call decodes at most (the work counter is 32 bits)

struct RangeDesc {             // must match snappy_hip_range (include/snappy_hip.h)
    uint64_t offset;
    uint64_t length;
    uint8_t* dst;
    uint32_t stream;
    uint32_t pad;
};

// Scratch of one call: the piece prefix (range_count + 2 u64: [r] = first piece of range r, [range_count] = all pieces,
// [range_count + 1] = pieces to decode), rounded up to 256 bytes, then one slot per wavefront.
__host__ __device__ inline uint64_t range_prefix_bytes(uint32_t range_count) { return round256(((uint64_t)range_count + 2u) * 8u); }
__host__ __device__ inline uint64_t range_slot_bytes(uint32_t max_block_size) { return round256(max_block_size); }

// Pieces of one range, or ~0 for a malformed request: a stream index >= count, offset + length beyond the container (or
// overflowing), a block size of 0 or above max_block_size (the slot holds no more), an index of too few blocks.
__device__ __forceinline__ uint64_t range_pieces(const StreamDesc* __restrict__ descs, uint32_t count, const RangeDesc& q, uint32_t max_block_size)
{
    if (q.stream >= count) return ~0ull;
    const StreamDesc d = descs[q.stream];
    const uint64_t end = q.offset + q.length;
    if (end < q.offset || end > d.total_len) return ~0ull;
    if (q.length == 0) return 0;
    if (d.block_size == 0 || d.block_size > max_block_size || q.dst == nullptr) return ~0ull;
    const uint64_t first = q.offset / d.block_size, last = (end - 1) / d.block_size;
    if (last >= d.num_blocks) return ~0ull;
    return last - first + 1;
}

// (SNAPPY_HIP_NO_KERNELS, snappy_kernels.hpp: another source of the library takes RangeDesc and the pieces above without the kernels)
#ifndef SNAPPY_HIP_NO_KERNELS

__global__ __launch_bounds__(1024) void range_pieces_kernel(const StreamDesc* __restrict__ descs, uint32_t count,
                                                            const RangeDesc* __restrict__ ranges, uint32_t range_count,
                                                            uint32_t* __restrict__ status, uint32_t max_block_size,
                                                            uint64_t* __restrict__ prefix)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint64_t cut_s;      // pieces to decode when there are more than kMaxRangePieces
    const uint32_t tid = threadIdx.x;

    uint64_t carry = 0;
    for (uint32_t base = 0; base < range_count; base += 1024) {
        const uint32_t i = base + tid;
        uint64_t mine = 0;
        bool bad = false;
        if (i < range_count) {
            const uint64_t n = range_pieces(descs, count, ranges[i], max_block_size);
            bad = n == ~0ull;
            mine = bad ? 0 : n;
        }
        uint64_t total;
        const uint64_t first = carry + workgroup_exclusive_scan(mine, wave_sums, total);
        if (i < range_count) {
            prefix[i] = first;
            // past kMaxRangePieces: the range that straddles it (exactly one when there are more pieces) marks the cut
            const bool beyond = first + mine > kMaxRangePieces;
            if (beyond && first <= kMaxRangePieces) cut_s = first;
            status[i] = (bad || beyond) ? kRangeOutOfBounds : kBlockOk;
        }
        carry += total;
    }
    __syncthreads();                // (cut_s, whichever trip wrote it)
    if (tid == 0) {
        prefix[range_count] = carry;
        prefix[range_count + 1] = carry > kMaxRangePieces ? cut_s : carry;
    }
}

__global__ __launch_bounds__(64) void decompress_ranges_kernel(const StreamDesc* __restrict__ descs, const RangeDesc* __restrict__ ranges,
                                                               uint32_t range_count, uint32_t* __restrict__ status,
                                                               const uint64_t* __restrict__ prefix, uint8_t* __restrict__ slots,
                                                               uint32_t slot_bytes, uint32_t* next_piece)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage_mem[kK2StageBytes];   // one window's output (K2's stage)
    lds_bytes_t stage = (lds_bytes_t)stage_mem;
    const uint32_t lane = threadIdx.x;
    const uint64_t pieces = prefix[range_count + 1];
    uint8_t* slot = slots + (uint64_t)blockIdx.x * slot_bytes;

    for (;;) {
        const uint32_t p = draw_work(next_piece, lane);
        if (p >= pieces) break;
        const uint32_t r = prefix_owner<true>(prefix, range_count, p);
        const RangeDesc q = ranges[r];
        const StreamDesc d = descs[q.stream];
        // validated by range_pieces_kernel: offset + length <= total_len < 4 GiB, block_size in [1, max_block_size]
        const uint8_t* stream = load_global_ptr(&descs[q.stream].stream);
        uint8_t* dst = load_global_ptr(&ranges[r].dst);
        const uint32_t bs = d.block_size;
        const uint32_t r_begin = (uint32_t)q.offset, r_end = (uint32_t)(q.offset + q.length);
        const uint32_t b = r_begin / bs + (p - (uint32_t)uld64(reinterpret_cast<const uint8_t*>(prefix + r)));
        const uint32_t ostart = b * bs;
        const uint32_t out_len = d.total_len - ostart < bs ? d.total_len - ostart : bs;
        const uint64_t at = uld64(reinterpret_cast<const uint8_t*>(load_global_ptr(&descs[q.stream].block_offsets) + b));
        uint32_t st;
        if (ostart >= r_begin && ostart + out_len <= r_end) {
            // whole piece: in place, as K2 writes a block at out + b * block_size
            st = k2_decode_block(stream, d.stream_len, at, dst + (ostart - r_begin), out_len, stage);
        } else {
            // partial piece: the whole block into this wavefront's slot, then the intersection out
            st = k2_decode_block(stream, d.stream_len, at, slot, out_len, stage);
            if (st == kBlockOk) {
                stores_landed();                                         // (the decode's)
                const uint32_t from = r_begin > ostart ? r_begin : ostart;
                const uint32_t to = r_end < ostart + out_len ? r_end : ostart + out_len;
                const uint32_t n = to - from;
                const uint8_t* s = slot + (from - ostart);
                uint8_t* t = dst + (from - r_begin);
                wave_copy(t, s, n, lane);
            }
        }
        if (st != kBlockOk && lane == 0) atomicOr(status + r, kBlockInvalid);
        __syncthreads();
    }
}

#endif  // SNAPPY_HIP_NO_KERNELS

}  // namespace snappy_hip
