// snappy_sz_ranges.hpp -- byte ranges of .sz streams decoded from a RESIDENT chunk index, without the rest of the streams
// (snappy_hip_sz_index_batch, snappy_hip_sz_decompress_ranges, include/snappy_hip.h).
//
// The chunks of a .sz stream are as independent as a container's blocks, but of variable length: a byte of the plaintext is found
// by a search over the chunks' output offsets, not by a division.  Two calls:
//   * the index: the split walk of snappy_sz_split.hpp (its steps 1 to 6, enqueued by snappy_hip_sz_split.hip over this call's
//     scratch) on SHADOW items -- sz_shadow_items_kernel gives every item a non-null dummy dst and the largest capacity, so that
//     the join's verdict never is DST_TOO_SMALL and the record step passes no item by; nothing is decoded -- then
//     sz_index_export_kernel: the records to the caller's array, a SzDesc per item.
//   * the ranges: a PIECE is a pair (range r, data chunk k) for every chunk k in first..last of the range, first / last = the
//     largest k with dst_off[k] <= offset / <= offset + length - 1.  sz_range_pieces_kernel (one workgroup, the shape of
//     range_pieces_kernel) validates every range, runs the two searches and scans the piece counts; sz_decompress_ranges_kernel
//     (persistent wavefronts, decompress_ranges_kernel's trip with sz_decode_chunks_kernel's decode and CRC) decodes a piece in
//     place when it lies wholly inside the range, else into the wavefront's slot, from which the intersection is copied; the
//     verdict of a range is a 64-bit atomicMin of (chunk << 32 | status) over its bad pieces, which sz_range_finish_kernel
//     unpacks: the lowest-numbered bad chunk, whatever the order of the wavefronts.
// THE INDEX IS NOT TRUSTED.  It is the caller's memory, and so are the streams.  Before a piece is decoded its record is held to
// the desc and to the stream: the chunk lies inside [src, src + src_len), the header re-read at src_off has the record's type and
// L, a compressed chunk's varint re-read there has the record's length and ulen, an uncompressed chunk's ulen is L - 4, and ulen
// is at most 65,536 (the slot).  A record that fails is BLOCK_INVALID for its piece.  What is written is decided per piece from
// the record's own dst_off and ulen against the range: in place only if [dst_off, dst_off + ulen) lies inside the range, else
// into the slot and the (possibly empty) intersection out.  So nothing outside [dst, dst + length) is written and nothing
// outside [src, src + src_len) is read, whatever records and streams hold; only the answers depend on them.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_ranges.hpp"      // RangeDesc, kMaxRangePieces, range_prefix_bytes
#include "snappy_sz.hpp"          // SzChunk, the statuses, k2_decode_block, crc32c_wave

namespace snappy_hip {

struct SzDesc {                // must match snappy_hip_sz_desc (include/snappy_hip.h)
    const uint8_t* src;
    uint64_t src_len;
    const SzChunk* chunks;
    uint64_t num_chunks;
    uint64_t total_len;
};
static_assert(sizeof(SzDesc) == 40, "SzDesc layout");

constexpr uint32_t kSzRangeSlotBytes = kSzMaxChunk;    // one chunk's plaintext
constexpr uint64_t kSzNoVerdict = ~0ull;

// Scratch of the index call, every part rounded up to 256 bytes: the shadow items, out_len[count], then the split walk's scratch.
struct SzIndexLayout {
    uint64_t out_len, split, total;
};
__host__ __device__ inline SzIndexLayout sz_index_layout(uint32_t count, uint64_t split_total)
{
    SzIndexLayout l;
    l.out_len = round256((uint64_t)count * sizeof(RawItem));
    l.split = l.out_len + round256((uint64_t)count * 8u);
    l.total = l.split + split_total;
    return l;
}

// Scratch of the range call: the piece prefix (range_count + 2 u64, as snappy_ranges.hpp), first[range_count] (u64: the first
// chunk of range r), verdict[range_count] (u64), then one slot of kSzRangeSlotBytes per wavefront.
struct SzRangeLayout {
    uint64_t first, verdict, slots;
};
__host__ __device__ inline SzRangeLayout sz_range_layout(uint32_t range_count)
{
    SzRangeLayout l;
    l.first = range_prefix_bytes(range_count);
    l.verdict = l.first + round256((uint64_t)range_count * 8u);
    l.slots = l.verdict + round256((uint64_t)range_count * 8u);
    return l;
}

// ---- the index ----
__global__ __launch_bounds__(256) void sz_shadow_items_kernel(const RawItem* __restrict__ items, uint32_t count, RawItem* __restrict__ shadow,
                                                              uint8_t* dummy)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
        RawItem q = items[i];
        q.dst = dummy;                                                   // (never written: nothing is decoded)
        q.dst_capacity = kRawMaxLen;
        shadow[i] = q;
    }
}

// Thread t < count: the desc of item t (an item that is not OK has no chunks and no length) and result[1]; thread t < the
// recorded chunks: record t to the caller's array, its last word 0.
__global__ __launch_bounds__(256) void sz_index_export_kernel(const RawItem* __restrict__ items, uint32_t count, const uint32_t* __restrict__ ctl,
                                                              const uint64_t* __restrict__ prefix, const SzChunk* __restrict__ chunks,
                                                              const uint64_t* __restrict__ out_len, const uint32_t* __restrict__ status,
                                                              SzChunk* __restrict__ out_chunks, SzDesc* __restrict__ descs,
                                                              uint32_t* __restrict__ result)
{
    const uint32_t recorded = ctl[kSzCtlChunks];
    const uint32_t units = recorded > count ? recorded : count;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < units; t += gridDim.x * 256u) {
        if (t < count) {
            const bool ok = status[t] == kBlockOk;
            SzDesc d;
            d.src = items[t].src;
            d.src_len = items[t].src_len;
            d.chunks = out_chunks + prefix[t];
            d.num_chunks = ok ? prefix[t + 1] - prefix[t] : 0;
            d.total_len = ok ? out_len[t] : 0;
            descs[t] = d;
            if (ok) atomicAdd(result + 1, 1u);
        }
        if (t < recorded) {
            SzChunk c = chunks[t];
            c.status = 0;                                                // (the reserved word)
            out_chunks[t] = c;
        }
    }
}

// ---- the ranges ----
// the largest k < n with chunks[k].dst_off <= x, or n if there is none; 32-byte strided dependent loads
__device__ __forceinline__ uint64_t sz_chunk_at(const SzChunk* __restrict__ chunks, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (chunks[mid].dst_off <= x) lo = mid;
        else hi = mid;
    }
    return chunks[lo].dst_off <= x ? lo : n;
}

// Pieces of one range and its first chunk, or ~0 for a malformed request: a stream index >= count, offset + length beyond the
// plaintext (or overflowing), a null dst, a desc without chunks, of 2^32 chunks or more, or without a chunk at the range's start.
__device__ __forceinline__ uint64_t sz_range_pieces(const SzDesc* __restrict__ descs, uint32_t count, const RangeDesc& q, uint64_t& first_out)
{
    first_out = 0;
    if (q.stream >= count) return ~0ull;
    const SzDesc d = descs[q.stream];
    const uint64_t end = q.offset + q.length;
    if (end < q.offset || end > d.total_len) return ~0ull;
    if (q.length == 0) return 0;
    if (q.dst == nullptr || d.chunks == nullptr || d.num_chunks == 0 || d.num_chunks > 0xffffffffull) return ~0ull;
    const SzChunk* chunks = load_global_ptr(&descs[q.stream].chunks);
    const uint64_t first = sz_chunk_at(chunks, d.num_chunks, q.offset);
    if (first == d.num_chunks) return ~0ull;
    const uint64_t last = sz_chunk_at(chunks, d.num_chunks, end - 1);       // (>= first: the same search for a larger value)
    if (last == d.num_chunks || last < first) return ~0ull;
    first_out = first;
    return last - first + 1;
}

__global__ __launch_bounds__(1024) void sz_range_pieces_kernel(const SzDesc* __restrict__ descs, uint32_t count, const RangeDesc* __restrict__ ranges,
                                                               uint32_t range_count, uint32_t* __restrict__ status, uint64_t* __restrict__ prefix,
                                                               uint64_t* __restrict__ first_chunk, uint64_t* __restrict__ verdict)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint64_t cut_s;      // pieces to decode when there are more than kMaxRangePieces
    const uint32_t tid = threadIdx.x;

    uint64_t carry = 0;
    for (uint32_t base = 0; base < range_count; base += 1024) {
        const uint32_t i = base + tid;
        uint64_t mine = 0, k0 = 0;
        bool bad = false;
        if (i < range_count) {
            const uint64_t n = sz_range_pieces(descs, count, ranges[i], k0);
            bad = n == ~0ull;
            mine = bad ? 0 : n;
        }
        uint64_t total;
        const uint64_t first = carry + workgroup_exclusive_scan(mine, wave_sums, total);
        if (i < range_count) {
            prefix[i] = first;
            first_chunk[i] = k0;
            verdict[i] = kSzNoVerdict;
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

// amdgpu_num_sgpr: the most scalar registers at which the compiler still counts eight wavefronts per SIMD for this kernel.  With
// the two window loops of k2_decode_block it would take 105; the ones beyond the cap live in lanes of a vector register.
template <int kTables>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_sgpr(102))) void sz_decompress_ranges_kernel(const SzDesc* __restrict__ descs, const RangeDesc* __restrict__ ranges,
                                                                  uint32_t range_count, uint32_t flags, const uint64_t* __restrict__ prefix,
                                                                  const uint64_t* __restrict__ first_chunk, uint64_t* verdict,
                                                                  uint8_t* __restrict__ slots, uint32_t* next_piece)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage_mem[kK2StageBytes];   // one window's output (K2's stage)
    __shared__ uint32_t table[crc_table_words<kTables>()];
    lds_bytes_t stage = (lds_bytes_t)stage_mem;
    const uint32_t lane = threadIdx.x;
    crc_table_init<kTables>(table, lane);
    __syncthreads();
    const uint64_t pieces = uld64(reinterpret_cast<const uint8_t*>(prefix + range_count + 1));
    uint8_t* slot = slots + (uint64_t)blockIdx.x * kSzRangeSlotBytes;

    for (;;) {
        const uint32_t p = draw_work(next_piece, lane);
        if (p >= pieces) break;
        const uint32_t r = prefix_owner<true>(prefix, range_count, p);
        const uint8_t* rq = reinterpret_cast<const uint8_t*>(ranges + r);
        const uint64_t r_begin = uld64(rq), r_end = r_begin + uld64(rq + 8);     // (validated: no overflow, <= total_len)
        const uint32_t s = uld32(rq + 24);
        uint8_t* dst = load_global_ptr(&ranges[r].dst);
        const uint8_t* src = load_global_ptr(&descs[s].src);
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&descs[s].src_len));
        const SzChunk* chunks = load_global_ptr(&descs[s].chunks);
        const uint64_t k = uld64(reinterpret_cast<const uint8_t*>(first_chunk + r)) + (p - uld64(reinterpret_cast<const uint8_t*>(prefix + r)));
        const uint8_t* rec = reinterpret_cast<const uint8_t*>(chunks + k);       // (k <= last < num_chunks: the planner's search)
        const uint64_t src_off = uld64(rec), dst_off = uld64(rec + 8);
        const uint32_t info = uld32(rec + 16), ulen = uld32(rec + 20);
        const uint32_t L = info & 0xffffffu, hdr = (info >> 24) & 15u;
        const bool compressed = (info & kSzInfoCompressed) != 0;

        // the record held to the desc and to the stream's own bytes
        uint32_t st = kBlockOk;
        if (ulen > kSzMaxChunk || (info >> 29) || L < 4u + hdr || src_off > src_len || 4ull + L > src_len - src_off) {
            st = kBlockInvalid;
        } else if (uld32(src + src_off) != ((L << 8) | (compressed ? 0u : 1u))) {
            st = kBlockInvalid;
        } else if (!compressed) {
            if (hdr != 0 || ulen != L - 4u) st = kBlockInvalid;
        } else {
            // the varint, by sz_walk's rules: hdr bytes inside the chunk that state ulen
            uint32_t length = 0, got = 0;
            for (uint32_t j = 0; j < 5 && j < hdr; ++j) {
                const uint32_t c = uni((uint32_t)src[src_off + 8 + j]);
                if (j == 4 && c >= 16u) break;
                length |= (c & 0x7fu) << (7u * j);
                if (c < 0x80u) {
                    got = j + 1;
                    break;
                }
            }
            if (got == 0 || got != hdr || length != ulen) st = kBlockInvalid;
        }

        if (st == kBlockOk) {
            const uint8_t* body = src + src_off;
            const uint32_t payload = L - 4u;
            const bool whole = dst_off >= r_begin && dst_off <= r_end && ulen <= r_end - dst_off;
            uint8_t* out = whole ? dst + (dst_off - r_begin) : slot;
            if (compressed) {
                if (ulen == 0) st = payload == hdr ? kBlockOk : kBlockInvalid;  // nothing may follow the header
                else st = k2_decode_block<true>(body + 8, payload, hdr, out, ulen, stage);
            } else {
                wave_copy(out, body + 8, ulen, lane);
            }
            if (st == kBlockOk && (!whole || !(flags & kSzNoVerify))) stores_landed();
            if (st == kBlockOk && !(flags & kSzNoVerify)) {
                const uint32_t crc = ~crc32c_wave<kTables>(0xffffffffu, out, ulen, lane, table);
                if (crc_mask(crc) != uld32(body + 4)) st = kSzCrcMismatch;
            }
            if (!whole && st != kBlockInvalid) {
                // partial piece: the intersection out of the slot (none, if the record's dst_off is not the range's)
                const uint64_t c_end = dst_off + ulen;
                const uint64_t from = r_begin > dst_off ? r_begin : dst_off;
                const uint64_t to = r_end < c_end ? r_end : c_end;
                if (from < to) wave_copy(dst + (from - r_begin), slot + (from - dst_off), (uint32_t)(to - from), lane);
            }
        }
        if (st != kBlockOk && lane == 0) atomicMin(reinterpret_cast<unsigned long long*>(verdict + r), (unsigned long long)((k << 32) | st));
        __syncthreads();
    }
}

// thread r: an OK range with a verdict takes the status and the chunk of its lowest-numbered bad piece
__global__ __launch_bounds__(256) void sz_range_finish_kernel(uint32_t range_count, const uint64_t* __restrict__ verdict, uint32_t* __restrict__ status,
                                                              uint32_t* __restrict__ bad_chunk)
{
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < range_count; r += gridDim.x * 256u) {
        uint32_t bad = 0xffffffffu;
        const uint64_t v = verdict[r];
        if (status[r] == kBlockOk && v != kSzNoVerdict) {
            status[r] = (uint32_t)v;
            bad = (uint32_t)(v >> 32);
        }
        bad_chunk[r] = bad;
    }
}

}  // namespace snappy_hip
