// snappy_sz_split.hpp -- the chunk chain of ONE large .sz stream walked by many wavefronts (snappy_hip_sz_decompress_split_batch,
// include/snappy_hip.h).
//
// sz_index_kernel (snappy_sz.hpp) gives a whole stream to one wavefront: 32,768 dependent chunk headers for 1 GiB, which is nearly
// all of the call.  A chunk's record needs only where the chunk starts, its number in the item and the output in front of it; so
// the stream is cut into SEGMENTS of segment_bytes compressed bytes, every segment finds a chunk start in its share and walks
// from there to the next segment's, and one lookup per segment joins them -- the layout of the raw split check
// (snappy_raw_check_split.hpp), with sz_walk's tests for the per-chunk ones.
//
// One phased call, each step a launch of its own (no kernel waits on another workgroup):
//   1 sz_split_plan_kernel     one workgroup: the items settled before any walk (a null src, src_len above kRawMaxLen); an item is
//                              LARGE when src_len > segment_bytes; the exclusive prefix of the large items' segments; the first
//                              large item that does not fit max_segments and every large one behind it are walked serially.
//   2 sz_split_anchor_kernel   a wavefront per segment: segment 0's ANCHOR is offset 0; every other segment scans its share 64
//                              positions at a time for the first that looks like a chunk start (sz_anchor_size) and from which
//                              kSzAnchorChain more such chunks follow or the stream ends; at most kSzAnchorTries candidates.
//   3 sz_split_walk_kernel     a wavefront per anchored segment: sz_walk's tests chunk by chunk from the anchor (segment 0 not
//                              yet identified, the others identified) until it LANDS EXACTLY on a later segment's anchor, reaches
//                              src_len, or meets a chunk sz_walk refuses.  Leaves its link, its data chunks, their bytes, an error.
//   4 sz_split_join_kernel     a wavefront per item: follows the links from segment 0; the item is PROVEN iff that path reaches
//                              src_len and no walker on it saw an error; every path segment gets its first chunk number and
//                              output offset.  Every other item that is not settled is walked by sz_walk, as sz_index_kernel
//                              does it.  The verdict logic is sz_index_kernel<false>'s, word for word.
//   5 sz_plan_kernel           (snappy_sz.hpp, unchanged) the chunks' prefix over the items and the max_chunks cut.
//   6 sz_split_record_kernel   the path's walkers again, each recording its chunks at chunks[item's first + segment's first + k]
//                              with dst_off = the segment's output base + its running sum; serial items by sz_walk<true>.
//   7, 8                       sz_decode_chunks_kernel and sz_finish_kernel, unchanged.
//
// WHY IT IS EXACT.  A walker applies sz_walk's tests to the chunk at its cursor and moves by 4 + L, as sz_walk does.  The path
// from segment 0 starts at offset 0 not identified, which is sz_walk's start; each of its walkers ends exactly where the next
// begins, and "identified" is true from the first chunk on (the first chunk is refused otherwise), which is what the later
// walkers start with.  So the path's chunks, in order, ARE the chunks sz_walk visits; if none was refused and the path ends at
// src_len, sz_walk's verdict is OK with the path's sums as its count and length.  A FALSE anchor -- a position that is not a
// chunk start of the true chain -- is never landed on by the true chain, because the true chain only ever stands on its own
// chunk starts: a walker on the path passes it by and stops at a later, true one (or the end).  A walker that starts at a false
// anchor is not on the path and is ignored.  So every large item with a valid chain inside max_segments is proven whatever the
// anchors are, and only the time depends on them; an item that is not proven is judged by sz_walk itself, whose verdict --
// which of UNSUPPORTED and INVALID comes first in chain order included -- is therefore the answer for every invalid chain.
// All cursors fit 32 bits under kRawMaxLen.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_sz.hpp"          // SzChunk, sz_walk, SzDecodeLayout, the statuses

namespace snappy_hip {

constexpr uint32_t kSzSplitDefaultSegment = 1u << 20;
constexpr uint32_t kSzSplitMinSegment = 256;
constexpr uint64_t kSzSplitMaxSegments = 1ull << 31;    // (the control word is 32 bits)
constexpr uint32_t kSzNone = 0xffffffffu;               // no anchor / no link
constexpr uint32_t kSzLinkEnd = 0xfffffffeu;            // the walker reached src_len
constexpr uint32_t kSzAnchorTries = 64;                 // candidates one share tries at most
constexpr uint32_t kSzAnchorChain = 4;                  // plausible chunks that must follow a candidate

enum : uint32_t { kSzCtlSegments = 1 };                 // word of the control line: the segments inside max_segments
// an item's flag word: its class, "walk it serially" (beyond max_segments, or not proven), "the parallel walk proved it"
enum : uint32_t { kSzItemDone = 0, kSzItemSmall = 1, kSzItemLarge = 2, kSzItemClassMask = 3, kSzItemSerial = 4, kSzItemProven = 8 };

// one segment of a large item
struct SzSeg {
    uint32_t anchor;           // offset in the item's src of the chunk start its walker begins at; kSzNone: no walker
    uint32_t link;             // the item's segment whose anchor the walker landed on, kSzLinkEnd, or kSzNone
    uint32_t chunks;           // data chunks the walker passed
    uint32_t err;              // it met a chunk sz_walk refuses
    uint64_t bytes;            // the sum of their uncompressed lengths
    uint64_t out_base;         // on the path: the item's output in front of the segment's first chunk
    uint32_t chunk_base;       // on the path: the item's data chunks in front of it
    uint32_t on_path;
};
static_assert(sizeof(SzSeg) == 40, "SzSeg layout (the kernels read its words by offset)");

// Scratch of one call, every part rounded up to 256 bytes: the parts of SzDecodeLayout (control line, prefix, chunks), then
// seg_prefix[count + 1] (u64: first segment of item i among the large items'), flags[count], segs[max_segments].
struct SzSplitLayout {
    SzDecodeLayout d;
    uint64_t seg_prefix, flags, segs, total;
};
__host__ __device__ inline SzSplitLayout sz_split_layout(uint32_t count, uint32_t max_chunks, uint64_t max_segments)
{
    if (max_segments > kSzSplitMaxSegments) max_segments = kSzSplitMaxSegments;
    SzSplitLayout l;
    l.d = sz_decode_layout(count, max_chunks);
    l.seg_prefix = l.d.total;
    l.flags = l.seg_prefix + round256(((uint64_t)count + 1u) * 8u);
    l.segs = l.flags + round256((uint64_t)count * 4u);
    l.total = l.segs + round256(max_segments * sizeof(SzSeg));
    return l;
}

// ---- 1: plan ----
__global__ __launch_bounds__(1024) void sz_split_plan_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t segment_bytes,
                                                             uint64_t max_segments, uint64_t* __restrict__ out_len, uint32_t* __restrict__ status,
                                                             uint32_t* __restrict__ result, uint32_t* __restrict__ ctl, uint64_t* __restrict__ prefix,
                                                             uint64_t* __restrict__ seg_prefix, uint32_t* __restrict__ flags)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint64_t cut_s;      // segments in front of the first item beyond the limit
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < count; base += 1024) {
        const uint32_t i = base + tid;
        uint64_t segs = 0;
        uint32_t flag = kSzItemDone;
        if (i < count) {
            const RawItem q = items[i];
            if (!q.src || q.src_len > kRawMaxLen) {                  // sz_index_kernel's two verdicts in front of the walk
                status[i] = !q.src ? kBlockInvalid : kRawTooLarge;
                out_len[i] = 0;
                prefix[i] = 0;
            } else if (q.src_len > segment_bytes) {
                flag = kSzItemLarge;
                segs = (q.src_len + segment_bytes - 1u) / segment_bytes;
            } else {
                flag = kSzItemSmall;
            }
        }
        uint64_t total;
        const uint64_t first = carry + workgroup_exclusive_scan(segs, wave_sums, total);
        if (i < count) {
            seg_prefix[i] = first;
            // past the limit: the first such item (exactly one starts inside it) marks the end of the work
            if (segs && first + segs > max_segments) {
                flag |= kSzItemSerial;
                if (first <= max_segments) cut_s = first;
            }
            flags[i] = flag;
        }
        carry += total;
    }
    __syncthreads();                // (cut_s, whichever trip wrote it)
    if (tid == 0) {
        seg_prefix[count] = carry;
        ctl[kSzCtlSegments] = (uint32_t)(carry <= max_segments ? carry : cut_s);
        result[2] = result[3] = 0;  // (sz_plan_kernel writes [0] and [1])
    }
}

// ---- 2: anchors ----
// Does a chunk start at `at`, as far as its own bytes tell?  Its size (4 + L), or 0.  Any lane, any position below src_len; reads
// nothing outside the chunk it accepts.  Skippable types are refused: at a random position they pass half the time.
__device__ __forceinline__ uint32_t sz_anchor_size(const uint8_t* src, uint32_t src_len, uint32_t at)
{
    if (src_len - at < 4u) return 0;
    const uint32_t w = ld32(src + at);
    const uint32_t type = w & 0xffu, L = w >> 8;
    if (L > src_len - at - 4u) return 0;                             // the chunk must fit
    if (type == 0xffu) return (L == 6 && ld32(src + at + 4) == 0x50614e73u && src[at + 8] == 0x70u && src[at + 9] == 0x59u) ? 10u : 0u;
    if (type == 1u) return (L >= 4u && L <= kSzMaxChunk + 4u) ? L + 4u : 0u;
    if (type != 0u || L < 5u) return 0;
    uint32_t u = 0, hdr = 0;                                         // the varint, by sz_walk's rules
    for (uint32_t k = 0; k < 5 && k < L - 4; ++k) {
        const uint32_t c = src[at + 8 + k];
        if (k == 4 && c >= 16u) break;
        u |= (c & 0x7fu) << (7u * k);
        if (c < 0x80u) {
            hdr = k + 1;
            break;
        }
    }
    if (hdr == 0 || u > kSzMaxChunk) return 0;
    const uint32_t elements = L - 4u - hdr;
    if (elements > 32u + u + u / 6u) return 0;                       // more than any compressor writes for u bytes
    if (u && (elements == 0 || (src[at + 8 + hdr] & 3u) != 0)) return 0;   // output starts with a literal
    return L + 4u;
}

__global__ __launch_bounds__(64) void sz_split_anchor_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t segment_bytes,
                                                             const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ seg_prefix,
                                                             SzSeg* __restrict__ segs)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t segments = uni(ctl[kSzCtlSegments]);
    for (uint32_t p = blockIdx.x; p < segments; p += gridDim.x) {
        const uint32_t i = prefix_owner<true>(seg_prefix, count, p);
        const uint32_t s = p - (uint32_t)uld64(reinterpret_cast<const uint8_t*>(seg_prefix + i));
        const uint8_t* src = load_global_ptr(&items[i].src);
        const uint32_t src_len = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
        uint32_t anchor = s == 0 ? 0u : kSzNone;
        if (s) {
            const uint32_t lo = s * segment_bytes, hi = src_len - lo < segment_bytes ? src_len : lo + segment_bytes;
            uint32_t tries = 0;
            for (uint32_t base = lo; base < hi && anchor == kSzNone && tries < kSzAnchorTries; base += kWave) {
                const uint32_t pos = base + lane;
                const uint32_t size = pos < hi ? sz_anchor_size(src, src_len, pos) : 0u;
                unsigned long long found = __ballot(size != 0);
                while (found && anchor == kSzNone && tries < kSzAnchorTries) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(found);
                    found &= found - 1;
                    ++tries;
                    // the chain from the candidate: kSzAnchorChain more plausible chunks, or the stream's end
                    uint32_t at = base + l + (uint32_t)__builtin_amdgcn_readlane((int)size, l);
                    bool ok = true;
                    for (uint32_t k = 0; k < kSzAnchorChain && at < src_len; ++k) {
                        const uint32_t n = uni(sz_anchor_size(src, src_len, at));
                        if (n == 0) {
                            ok = false;
                            break;
                        }
                        at += n;
                    }
                    if (ok) anchor = base + l;
                }
            }
        }
        if (lane == 0) {
            SzSeg r;
            r.anchor = anchor;
            r.link = kSzNone;
            r.chunks = r.err = 0;
            r.bytes = r.out_base = 0;
            r.chunk_base = r.on_path = 0;
            segs[p] = r;
        }
    }
}

// ---- 3 and 6: the walk of one segment ----
// sz_walk's trip from `start` (a chunk start in segment s of the item, `identified` as given) by every lane of a wavefront alike,
// until the cursor stands exactly on the anchor of another segment (link = that segment), on src_len (kSzLinkEnd), or at a chunk
// sz_walk refuses (err, link = kSzNone).  The per-chunk tests are sz_walk's, line for line; an anchor is looked up once per
// segment the cursor enters.  kRecord: lane 0 writes chunk k's record to rec[k] with dst_off = dst_base + the sum so far.
template <bool kRecord>
__device__ __forceinline__ void sz_split_walk(const uint8_t* src, uint64_t src_len, uint32_t segment_bytes, const SzSeg* item_segs, uint32_t s,
                                              uint32_t start, uint32_t& link_out, uint32_t& chunks_out, uint64_t& total_out, uint32_t& err_out,
                                              SzChunk* rec, uint64_t dst_base, uint32_t item, uint32_t lane)
{
    uint64_t at = start, total = 0;
    uint32_t chunks = 0, link = kSzNone, err = 0;
    bool identified = s != 0;
    uint64_t next_boundary = ((uint64_t)s + 1u) * segment_bytes;    // the end of the segment the cursor is in
    uint32_t here = s, here_anchor = kSzNone;                       // that segment and its anchor (the own one: never a stop)
    for (;;) {
        if (at >= src_len) {
            link = kSzLinkEnd;
            break;
        }
        if (at >= next_boundary) {
            here = (uint32_t)(at / segment_bytes);
            next_boundary = ((uint64_t)here + 1u) * segment_bytes;
            here_anchor = uld32(reinterpret_cast<const uint8_t*>(&item_segs[here].anchor));
        }
        if (here_anchor == at) {
            link = here;
            break;
        }
        err = 1;                                                     // (until the chunk has passed)
        if (at + 4 > src_len) break;
        const uint32_t w = uld32(src + at);
        const uint32_t type = w & 0xffu, L = w >> 8;
        if (at + 4 + L > src_len) break;                             // a chunk running past the stream
        if (type == 0xffu) {
            if (L != 6 || uld32(src + at + 4) != 0x50614e73u || uni((uint32_t)src[at + 8]) != 0x70u || uni((uint32_t)src[at + 9]) != 0x59u) break;
            identified = true;
        } else if (!identified) {                                    // the first chunk is not the identifier
            break;
        } else if (type <= 1u) {
            if (L < 4) break;
            uint32_t length = L - 4, hdr = 0;
            if (type == 0) {
                length = 0;
                for (uint32_t k = 0; k < 5 && k < L - 4; ++k) {
                    const uint32_t c = uni((uint32_t)src[at + 8 + k]);
                    if (k == 4 && c >= 16u) break;
                    length |= (c & 0x7fu) << (7u * k);
                    if (c < 0x80u) {
                        hdr = k + 1;
                        break;
                    }
                }
                if (hdr == 0) break;
            }
            if (length > kSzMaxChunk) break;                         // an oversized chunk
            if (kRecord && lane == 0) {
                SzChunk c;
                c.src_off = at;
                c.dst_off = dst_base + total;
                c.info = L | (hdr << 24) | (type == 0 ? kSzInfoCompressed : 0u);
                c.ulen = length;
                c.item = item;
                c.status = kBlockOk;
                rec[chunks] = c;
            }
            total += length;
            ++chunks;
        } else if (type < 0x80u) {                                   // reserved unskippable
            break;
        }                                                            // (0x80..0xfe: skipped)
        err = 0;
        at += 4ull + L;
    }
    link_out = link;
    chunks_out = chunks;
    total_out = total;
    err_out = err;
}

__global__ __launch_bounds__(64) void sz_split_walk_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t segment_bytes,
                                                           const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ seg_prefix, SzSeg* segs)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t segments = uni(ctl[kSzCtlSegments]);
    for (uint32_t p = blockIdx.x; p < segments; p += gridDim.x) {
        const uint32_t anchor = uld32(reinterpret_cast<const uint8_t*>(&segs[p].anchor));
        if (anchor == kSzNone) continue;
        const uint32_t i = prefix_owner<true>(seg_prefix, count, p);
        const uint64_t first = uld64(reinterpret_cast<const uint8_t*>(seg_prefix + i));
        const uint8_t* src = load_global_ptr(&items[i].src);
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
        uint32_t link, chunks, err;
        uint64_t total;
        sz_split_walk<false>(src, src_len, segment_bytes, segs + first, p - (uint32_t)first, anchor, link, chunks, total, err, nullptr, 0, i, lane);
        if (lane == 0) {
            segs[p].link = link;
            segs[p].chunks = chunks;
            segs[p].err = err;
            segs[p].bytes = total;
        }
    }
}

// ---- 4: join, and the serial walk of everything else ----
__global__ __launch_bounds__(64) void sz_split_join_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t max_chunks,
                                                           uint64_t* __restrict__ out_len, uint32_t* __restrict__ status, uint64_t* __restrict__ prefix,
                                                           SzChunk* __restrict__ chunks, const uint64_t* __restrict__ seg_prefix, uint32_t* flags,
                                                           SzSeg* segs, uint32_t* result)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t flag = uld32(reinterpret_cast<const uint8_t*>(flags + i));
        const uint32_t cls = flag & kSzItemClassMask;
        if (cls == kSzItemDone) continue;
        const uint8_t* src = load_global_ptr(&items[i].src);
        uint8_t* dst = load_global_ptr(&items[i].dst);
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
        const uint64_t capacity = dst ? uld64(reinterpret_cast<const uint8_t*>(&items[i].dst_capacity)) : 0;
        uint64_t total = 0;
        uint32_t n = 0, st = kBlockOk;
        bool proven = false;
        if (cls == kSzItemLarge && !(flag & kSzItemSerial)) {
            const uint64_t first = uld64(reinterpret_cast<const uint8_t*>(seg_prefix + i));
            const uint32_t nsegs = (uint32_t)(uld64(reinterpret_cast<const uint8_t*>(seg_prefix + i + 1)) - first);
            SzSeg* mine = segs + first;
            for (uint32_t cur = 0;;) {
                const uint8_t* r = reinterpret_cast<const uint8_t*>(mine + cur);
                const uint32_t anchor = uld32(r), link = uld32(r + 4), c = uld32(r + 8), err = uld32(r + 12);
                if (anchor == kSzNone || err) break;
                if (lane == 0) {
                    mine[cur].out_base = total;
                    mine[cur].chunk_base = n;
                    mine[cur].on_path = 1;
                }
                total += uld64(r + 16);
                n += c;
                if (link == kSzLinkEnd) {
                    proven = true;
                    break;
                }
                if (link <= cur || link >= nsegs) break;             // (kSzNone; a link only ever points forward)
                cur = link;
            }
        }
        if (!proven) {                                               // sz_index_kernel<false>'s walk
            if (i == 0) st = sz_walk<true>(src, src_len, total, n, chunks, max_chunks, i, lane);
            else st = sz_walk<false>(src, src_len, total, n, nullptr, 0, i, lane);
        }
        if (st != kBlockOk) total = 0;
        else if (total > kRawMaxLen) st = kRawTooLarge;
        else if (total > capacity) st = kRawDstTooSmall;
        if (lane == 0) {
            status[i] = st;
            out_len[i] = total;
            prefix[i] = st == kBlockOk ? n : 0u;
            flags[i] = flag | (proven ? kSzItemProven : kSzItemSerial);
            if (cls == kSzItemLarge) atomicAdd(result + (proven ? 2 : 3), 1u);
        }
    }
}

// ---- 6: record ----
// Work unit u < count: item u, if it was walked serially and is still OK, by sz_walk<true> (item 0 was recorded by step 4, as
// sz_index_kernel records it); unit count + p: segment p, if it is on the path of a proven item that is still OK.
__global__ __launch_bounds__(64) void sz_split_record_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t segment_bytes,
                                                             const uint32_t* __restrict__ ctl, const uint32_t* __restrict__ status,
                                                             const uint64_t* __restrict__ prefix, SzChunk* __restrict__ chunks,
                                                             const uint64_t* __restrict__ seg_prefix, const uint32_t* __restrict__ flags,
                                                             const SzSeg* __restrict__ segs)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t units = (uint64_t)count + uni(ctl[kSzCtlSegments]);
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        if (u < count) {
            const uint32_t i = (uint32_t)u;
            const uint32_t flag = uld32(reinterpret_cast<const uint8_t*>(flags + i));
            if (i == 0 || !(flag & kSzItemSerial) || uni(status[i]) != kBlockOk) continue;
            const uint8_t* src = load_global_ptr(&items[i].src);
            const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
            uint64_t total;
            uint32_t n;
            (void)sz_walk<true>(src, src_len, total, n, chunks + uld64(reinterpret_cast<const uint8_t*>(prefix + i)), 0xffffffffu, i, lane);
        } else {
            const uint32_t p = (uint32_t)(u - count);
            const uint8_t* r = reinterpret_cast<const uint8_t*>(segs + p);
            if (!uld32(r + 36)) continue;                            // on_path
            const uint32_t i = prefix_owner<true>(seg_prefix, count, p);
            const uint32_t flag = uld32(reinterpret_cast<const uint8_t*>(flags + i));
            if (!(flag & kSzItemProven) || uni(status[i]) != kBlockOk) continue;
            const uint64_t first = uld64(reinterpret_cast<const uint8_t*>(seg_prefix + i));
            const uint8_t* src = load_global_ptr(&items[i].src);
            const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
            SzChunk* rec = chunks + uld64(reinterpret_cast<const uint8_t*>(prefix + i)) + uld32(r + 32);
            uint32_t link, n, err;
            uint64_t total;
            sz_split_walk<true>(src, src_len, segment_bytes, segs + first, p - (uint32_t)first, uld32(r), link, n, total, err, rec, uld64(r + 24), i, lane);
        }
    }
}

}  // namespace snappy_hip
