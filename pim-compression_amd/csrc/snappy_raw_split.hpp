// snappy_raw_split.hpp -- ONE large raw Snappy stream decoded by many wavefronts, exactly
// (snappy_hip_raw_decompress_split_batch, include/snappy_hip.h).
//
// raw_decompress_kernel (snappy_raw.hpp) gives a whole stream to one wavefront, because element boundaries cannot be found
// without parsing the stream.  Real streams, though, are built from FRAGMENTS: Google's compressor, pyarrow and
// snappy_hip_raw_compress_batch compress fixed-size pieces of the plaintext independently, so at every multiple of the
// fragment size the output position coincides with an element start and no copy reaches back across it.  This call finds
// those element starts with many wavefronts and decodes every piece ("unit", unit_len output bytes) on its own.
//
// THE PROOF IS IN STEP 5 ALONE.  Unit k is decoded by the strict raw decoder, k2_decode_block<true>, from the compressed bytes
// [cut[k], cut[k + 1]) into dst[k * unit_len, ...) as if it were a stream of its own: every element must end inside those
// bytes, the output must be exactly the unit's length, and a copy that reaches before the unit's first byte is refused.  The
// kernel itself checks that cut[0] is the header's end, that the last cut is src_len and that the cuts ascend; neighbours
// share a cut.  So when every unit of an item is OK the units' elements, in order, ARE the item's element stream, every
// element passed tests at least as strict as the serial decoder's, every copy read bytes of its own unit that the same
// wavefront had written, and the outputs tile [0, length): the bytes are those of the serial decode and the verdict is OK.
// In every other case -- a cut missing, a unit refused, a damaged stream -- the item is marked and the serial decoder
// (step 6) gives it the authoritative verdict and bytes.  A mistake anywhere in steps 2-4 can therefore cause fallbacks,
// never a wrong byte, and nothing is ever written outside [dst, dst + length).
//
// One phased call, each step a kernel:
//   1 raw_split_plan_kernel    one workgroup: the header rules of raw_decompress_kernel (SNAPPY_RAW_ITEM_VERDICT), out_len and
//                              the header-level verdicts; items are classed done / small / split; exclusive prefixes of the
//                              split items' segments and units; the cut table set to NONE.
//   2 raw_split_walk_kernel    persistent wavefronts draw (item, segment).  A segment is segment_bytes compressed bytes from
//                              the header's end on.  Lane l walks the chain of elements that starts at the segment's byte l --
//                              sizes only, no payload -- to the first position at or beyond the next segment and stores
//                              (landing, output bytes).  The true chain enters a segment either in these first 64 bytes (the
//                              "zone": any element of up to 61 bytes that straddles the segment's start ends there) or behind a
//                              longer literal.
//   3 raw_split_resolve_kernel one wavefront per item follows the true chain from the header's end: an entry inside a zone is a
//                              table lookup, an entry behind it is walked (split_walk), an entry beyond a segment passes it by.
//                              One node (entry, landing, output base) per step, the output base as a running sum.  The item
//                              is "shaped" iff the chain ends exactly at src_len with the header's length as its sum.  THIS
//                              STEP IS SERIAL ALONG THE ITEM: one lookup per segment for streams of short elements, and the one
//                              part of the call whose time grows with the item whatever the device's width.
//   4 raw_split_cuts_kernel    persistent wavefronts, one node each: the node's elements are walked again, now with their
//                              output positions known, and every element that starts at a multiple of unit_len leaves its
//                              compressed position in cut[].
//   5 raw_split_units_kernel   persistent wavefronts draw (item, unit): see above.
//   6 raw_split_serial_kernel  raw_decompress_kernel's trip (SNAPPY_RAW_DECODE_ITEM) over the small items and the marked ones;
//                              the others get SNAPPY_HIP_BLOCK_OK.  Counts the three classes into d_result.
// split_walk is k2_check_block<true>'s window loop as a skeleton of its own once more (K2's code must not change by a single
// instruction): it starts anywhere, stops at the first element start at or beyond a given position, makes no copy-offset
// test -- where earlier output came from is another wavefront's business -- and can emit the cuts.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_kernels.hpp"   // window_issue, predecode_window, k2_chain_walk, k2_decode_block
#include "snappy_raw.hpp"       // RawItem, kRawMaxLen, SNAPPY_RAW_ITEM_VERDICT, SNAPPY_RAW_DECODE_ITEM

namespace snappy_hip {

constexpr uint32_t kSplitNone = 0xffffffffu;         // no cut / no node
constexpr uint64_t kSplitInvalid = ~0ull;            // a table entry whose chain met an invalid element
constexpr uint32_t kSplitZone = 64;                  // candidates per segment: one per lane
constexpr uint64_t kSplitMaxWork = 1ull << 31;       // segments / units one call takes at most (the work counters are 32 bits)
constexpr uint32_t kSplitDefaultUnit = 65536, kSplitDefaultSegment = 16384;   // (the segment: the best of 16 / 64 / 256 KiB)
constexpr uint32_t kSplitPending = 0xffffffffu;      // plan: "no verdict at header level"

// an item's flag word: bits 1:0 its class, bit 2 "decode it serially", bits 15:8 its header's length
enum : uint32_t { kSplitDone = 0, kSplitSmall = 1, kSplitSplit = 2, kSplitClassMask = 3, kSplitFallback = 4 };
// words of the control line at the start of the scratch
enum : uint32_t { kSplitCtlSegments = 0, kSplitCtlUnits = 1 };

// Scratch of one call, every part rounded up to 256 bytes: control line, seg_prefix[count + 1] and unit_prefix[count + 1]
// (u64: first segment / unit of item i among the split items'), flags[count], table[max_segments][64] (u64: landing | output
// bytes << 32), nodes[max_segments] (uint4: entry, landing, output base; the node of a step lives at the segment of its entry)
// and cuts[max_units + count] (u32; item i's units + 1 cuts start at unit_prefix[i] + i).
struct SplitLayout {
    uint64_t seg_prefix, unit_prefix, flags, table, nodes, cuts, total;
};
__host__ __device__ inline SplitLayout split_layout(uint32_t count, uint64_t max_segments, uint64_t max_units)
{
    if (max_segments > kSplitMaxWork) max_segments = kSplitMaxWork;
    if (max_units > kSplitMaxWork) max_units = kSplitMaxWork;
    SplitLayout l;
    l.seg_prefix = 256;
    l.unit_prefix = l.seg_prefix + round256(((uint64_t)count + 1u) * 8u);
    l.flags = l.unit_prefix + round256(((uint64_t)count + 1u) * 8u);
    l.table = l.flags + round256((uint64_t)count * 4u);
    l.nodes = l.table + round256(max_segments * kSplitZone * 8u);
    l.cuts = l.nodes + round256(max_segments * 16u);
    l.total = l.cuts + round256((max_units + count) * 4u);
    return l;
}

// Size of the element at src[pos] as predecode_window<true> sizes it, by ONE lane for itself: consumed = its compressed bytes,
// olen = its output bytes.  False where predecode_window rejects: a length field of 0xFFFFFFFF, or a header or a literal's
// payload running past src_len.  Reads the tag and at most four bytes behind it, never a byte at or beyond src_len.
__device__ __forceinline__ bool split_element_size(const uint8_t* src, uint64_t pos, uint64_t src_len, uint32_t& consumed, uint32_t& olen)
{
    uint64_t w = 0;
    if (pos + 8 <= src_len) {
        w = ld64(src + pos);
    } else {
        for (uint32_t k = 0; k < 5 && pos + k < src_len; ++k) w |= (uint64_t)src[pos + k] << (8 * k);
    }
    const uint32_t tag = (uint32_t)w & 0xffu;
    const uint32_t type = tag & 3u;
    const uint32_t v = tag >> 2;
    const uint32_t next4 = (uint32_t)(w >> 8);
    const bool lit = type == 0;
    const bool long_lit = lit && v >= 60u;
    const uint32_t raw = next4 & (0xffffffffu >> ((63u - v) * 8u & 31u));
    olen = long_lit ? raw + 1u : ((type == 1) ? (v & 7u) + 4u : v + 1u);
    const uint32_t hdr = long_lit ? v - 58u : (lit ? 1u : ((type == 3) ? 5u : type + 1u));
    const uint64_t payload = lit ? olen : 0u;
    consumed = hdr + (uint32_t)payload;
    return olen != 0 && pos + hdr + payload <= src_len;
}

// The elements of stream[entry, ...) walked by the whole wavefront, a 64-byte window at a time, up to the first element start
// at or beyond stop_at (entry < stop_at <= stream_len <= kRawMaxLen): `landing` = that start, op_end = op0 + the output bytes of
// the elements walked.  False when an element is invalid (as predecode_window<true> judges it against stream_len) or the
// output would pass `length`.  kEmit: every element walked whose output position is a multiple of unit_len stores its
// compressed position in cuts[position / unit_len].  kOffsets (the split check, snappy_raw_check_split.hpp): op0 is the entry's
// ABSOLUTE output position in the item, and every copy walked is tested as k2_check_block tests it -- false for an offset of 0
// or one larger than the copy's output position.  Wave-uniform arguments; every lane of the wavefront calls it.  The
// cursors are K2's, relative to `entry` (see k2_check_block); a long literal is skipped, its payload never loaded.
template <bool kEmit, bool kOffsets = false>
__device__ __forceinline__ bool split_walk(const uint8_t* stream, uint32_t stream_len, uint32_t entry, uint32_t stop_at, uint32_t op0,
                                           uint32_t length, uint32_t unit_len, uint32_t* cuts, uint32_t& landing, uint32_t& op_end)
{
    const uint32_t lane = threadIdx.x;
    const uint8_t* __restrict__ src = stream + entry;
    const uint32_t csz = stream_len - entry;
    const uint32_t limit = stop_at - entry;
    const uint64_t avail = csz;
    bool ok = true;

    uint32_t g = 0;
    uint32_t cp = 0, op = op0;
    uint64_t w0 = 0;
    WindowLoad next = {0, 64};
    WindowLoad next2 = {0, 64};
    bool have_window = false;
    const uint32_t avail32 = csz;
    bool next_tail = true, next2_tail = true;
    // the next multiple of unit_len at or behind op, and its number
    uint32_t next_k = kEmit ? (op0 + unit_len - 1u) / unit_len : 0u;
    uint32_t next_cut = next_k * unit_len;
    auto issue = [&](uint32_t base, bool& tail) -> WindowLoad {
        WindowLoad r;
        if (base + 72u <= avail32) {
            r.raw = ld64(src + (base + lane));
            r.shift = 0;
            tail = false;
        } else {
            r = window_issue(src, (uint64_t)base + lane, avail);
            tail = true;
        }
        return r;
    };
    while (cp < limit) {                                             // one iteration per 64-byte window
        if (!have_window) {
            g = cp & ~63u;
            bool cur_tail;
            const WindowLoad cur = issue(g, cur_tail);
            next = issue(g + 64u, next_tail);
            next2 = issue(g + 128u, next2_tail);
            w0 = cur_tail ? window_value(cur) : cur.raw;
            have_window = true;
        }
        const uint32_t wend = (limit < g + 64) ? limit : g + 64;     // element starts at or beyond `limit` are not this walk's
        const uint32_t wlim = wend - g;
        uint32_t e_type, e_hdr, e_len, e_consumed, offv;
        unsigned long long REJ;
        predecode_window<true>(w0, g + lane, csz, e_type, e_hdr, e_len, offv, e_consumed, REJ);
        const uint32_t advv = __builtin_amdgcn_inverse_ballot_w64(REJ) ? 64u : e_consumed;
        uint32_t s = cp - g;
        unsigned long long E = 0;
        {                                                            // the doubled jump vector and the fill-in, as K2 has them
            uint32_t jump[kK2WalkLevels + 1], tgt[kK2WalkLevels + 1];
            jump[0] = advv;
            tgt[0] = lane + advv;
#pragma unroll
            for (uint32_t k = 1; k <= kK2WalkLevels; ++k) {
                const uint32_t a_n = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(tgt[k - 1] << 2), (int)jump[k - 1]);
                jump[k] = jump[k - 1] + (tgt[k - 1] < wlim ? a_n : 0u);
                tgt[k] = lane + jump[k];
            }
            k2_chain_walk(jump[kK2WalkLevels], wlim, s, E);
#pragma unroll
            for (uint32_t k = kK2WalkLevels; k-- > 0;) {
                const bool pusher = __builtin_amdgcn_inverse_ballot_w64(E) && tgt[k] < wlim;
                const uint32_t got = (uint32_t)__builtin_amdgcn_ds_permute((int)(pusher ? tgt[k] << 2 : 0u), pusher ? 1 : 0);
                E |= __ballot(got != 0) & ~1ull;
            }
        }
        if (E & REJ) {                                               // an element predecode rejected
            ok = false;
            break;
        }
        const bool starts = __builtin_amdgcn_inverse_ballot_w64(E);
        const uint32_t mylen = starts ? e_len : 0u;
        const uint32_t incl = wave_inclusive_scan(mylen, lane);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (total > length - op) {                                   // (op <= length throughout)
            ok = false;
            break;
        }
        if constexpr (kOffsets) {
            const uint32_t dstp = op + (incl - mylen);               // where this lane's element starts in the item's output
            const unsigned long long COPY = E & __ballot(e_type != 0);
            if (COPY & (__ballot(offv == 0) | __ballot(offv > dstp))) {
                ok = false;
                break;
            }
        }
        if constexpr (kEmit) {
            if (op + total > next_cut) {                             // a multiple of unit_len inside this window's output
                const uint32_t dstp = op + (incl - mylen);           // where this lane's element starts in the item's output
                if (starts && dstp >= next_cut) {
                    const uint32_t d = dstp - next_cut;
                    const uint32_t q = d / unit_len;
                    if (q * unit_len == d) cuts[next_k + q] = entry + g + lane;
                }
                const uint32_t m = (op + total - next_cut + unit_len - 1u) / unit_len;
                next_k += m;
                next_cut += m * unit_len;                            // (< length + unit_len < 2^32)
            }
        }
        op += total;
        cp = g + s;
        if (cp < g + 128u) {
            SNAPPY_PIN(next.raw);
            SNAPPY_PIN(next2.raw);
            w0 = next_tail ? window_value(next) : next.raw;
            next = next2;
            next_tail = next2_tail;
            g += 64;
            next2 = issue(g + 128u, next2_tail);
        } else {
            have_window = false;                                     // a long literal: skipped, its payload is never loaded
        }
    }
    landing = entry + cp;
    op_end = op;
    return ok;
}

// The body of the segment walk (step 2), shared with the split check (snappy_raw_check_split.hpp), whose step 2 it is too: a
// macro for SNAPPY_RAW_ITEM_VERDICT's reason (snappy_raw.hpp).  The arguments are raw_split_walk_kernel's parameters.
#define SNAPPY_SPLIT_WALK_SEGMENTS(items, count, segment_bytes, ctl, seg_prefix, flags, table, nodes, next_segment)               \
    const uint32_t lane = threadIdx.x;                                                                                            \
    const uint32_t segments = uni(ctl[kSplitCtlSegments]);                                                                        \
    for (;;) {                                                                                                                    \
        const uint32_t p = draw_work(next_segment, lane);                                                                         \
        if (p >= segments) break;                                                                                                 \
        const uint32_t i = prefix_owner<false>(seg_prefix, count, p);                                                             \
        const uint8_t* src = load_global_ptr(&items[i].src);                                                                      \
        const uint64_t src_len = uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));     /* (validated: <= kRawMaxLen) */ \
        const uint32_t hdr = uni(flags[i]) >> 8;                                                                                  \
        const uint64_t s = p - uld64(reinterpret_cast<const uint8_t*>(seg_prefix + i));                                           \
        const uint64_t start = hdr + s * segment_bytes;                                                                           \
        const uint64_t end = start + segment_bytes < src_len ? start + segment_bytes : src_len;                                   \
        /* every lane a chain of its own: nothing below is wave-uniform, nothing in it talks to another lane */                   \
        uint64_t pos = start + lane, out = 0;                                                                                     \
        bool ok = true;                                                                                                           \
        while (pos < end) {                                                                                                       \
            uint32_t consumed, olen;                                                                                              \
            if (!split_element_size(src, pos, src_len, consumed, olen)) {                                                         \
                ok = false;                                                                                                       \
                break;                                                                                                            \
            }                                                                                                                     \
            pos += consumed;                                                                                                      \
            out += olen;                                                                                                          \
        }                                                                                                                         \
        if (out > kRawMaxLen) ok = false;                            /* (more than any header allows: no true chain) */           \
        table[(uint64_t)p * kSplitZone + lane] = ok ? (pos | (out << 32)) : kSplitInvalid;                                        \
        if (lane == 0) nodes[p] = make_uint4(kSplitNone, 0, 0, 0);   /* no step of the true chain starts here, until step 3 says so */\
        __syncthreads();            /* (the wavefront stays together from one draw to the next: see check_kernel) */              \
    }

// The true chain of item i followed from the header's end (step 3), one node per step, shared with the split check.  Declares
// src, src_len, length, hdr, first and `shaped` in the caller's scope.  i and flag (the item's flag word) are wave-uniform.
#define SNAPPY_SPLIT_RESOLVE_CHAIN(items, i, flag, unit_len, segment_bytes, out_len, seg_prefix, table, nodes, lane)              \
    const uint8_t* src = load_global_ptr(&items[i].src);                                                                          \
    const uint32_t src_len = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));                                \
    const uint32_t length = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(out_len + i));                                       \
    const uint32_t hdr = flag >> 8;                                                                                               \
    const uint64_t first = uld64(reinterpret_cast<const uint8_t*>(seg_prefix + i));                                               \
    uint32_t e = hdr, base = 0;                                                                                                   \
    bool ok = true;                                                                                                               \
    while (ok && e < src_len) {                                                                                                   \
        const uint32_t s = (e - hdr) / segment_bytes;                                                                             \
        const uint64_t zone = hdr + (uint64_t)s * segment_bytes;                                                                  \
        const uint64_t zend = zone + segment_bytes;                                                                               \
        const uint32_t end = zend < src_len ? (uint32_t)zend : src_len;                                                           \
        uint32_t landing, out;                                                                                                    \
        if (e - zone < kSplitZone) {                                                                                              \
            const uint64_t t = uld64(reinterpret_cast<const uint8_t*>(table + (first + s) * kSplitZone + (e - zone)));            \
            ok = t != kSplitInvalid;                                                                                              \
            landing = (uint32_t)t;                                                                                                \
            out = (uint32_t)(t >> 32);                                                                                            \
        } else {                                                 /* behind a literal longer than the zone */                      \
            uint32_t op_end;                                                                                                      \
            ok = split_walk<false>(src, src_len, e, end, base, length, unit_len, nullptr, landing, op_end);                       \
            out = op_end - base;                                                                                                  \
        }                                                                                                                         \
        if (!ok || out > length - base || landing <= e || landing > src_len) {                                                    \
            ok = false;                                                                                                           \
            break;                                                                                                                \
        }                                                                                                                         \
        if (lane == 0) nodes[first + s] = make_uint4(e, landing, base, 0);                                                        \
        base += out;                                                                                                              \
        e = landing;                                                                                                              \
    }                                                                                                                             \
    const bool shaped = ok && e == src_len && base == length;

#ifndef SNAPPY_HIP_NO_KERNELS
// ---- 1: plan ----
__global__ __launch_bounds__(1024) void raw_split_plan_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t unit_len,
                                                              uint32_t segment_bytes, uint64_t max_segments, uint64_t max_units,
                                                              uint64_t* __restrict__ out_len, uint32_t* __restrict__ status,
                                                              uint32_t* __restrict__ result, uint32_t* __restrict__ ctl,
                                                              uint64_t* __restrict__ seg_prefix, uint64_t* __restrict__ unit_prefix,
                                                              uint32_t* __restrict__ flags, uint32_t* __restrict__ cuts)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint64_t cut_s[2];   // segments / units in front of the first item beyond the limits
    const uint32_t tid = threadIdx.x;
    uint64_t carry_s = 0, carry_u = 0;
    for (uint32_t base = 0; base < count; base += 1024) {
        const uint32_t i = base + tid;
        uint64_t segs = 0, units = 0;
        uint32_t flag = kSplitDone;
        if (i < count) {
            SNAPPY_RAW_ITEM_VERDICT(items, i, ld64, uint32_t, kSplitPending)
            out_len[i] = length;
            if (st != kSplitPending) {
                status[i] = st;
            } else {
                const uint64_t s = (src_len - hdr + segment_bytes - 1u) / segment_bytes;
                flag = kSplitSmall | (hdr << 8);
                if (length > unit_len && s > 1) {                    // (else: one unit or one segment, nothing to split)
                    flag = kSplitSplit | (hdr << 8);
                    segs = s;
                    units = ((uint64_t)length + unit_len - 1u) / unit_len;
                }
            }
        }
        uint64_t total_s, total_u;
        const uint64_t first_s = carry_s + workgroup_exclusive_scan(segs, wave_sums, total_s);
        const uint64_t first_u = carry_u + workgroup_exclusive_scan(units, wave_sums, total_u);
        if (i < count) {
            seg_prefix[i] = first_s;
            unit_prefix[i] = first_u;
            // past the limits: the first such item (exactly one starts inside both of them) marks the end of the work
            const bool beyond = segs && (first_s + segs > max_segments || first_u + units > max_units);
            if (beyond) {
                flag |= kSplitFallback;
                if (first_s <= max_segments && first_u <= max_units) {
                    cut_s[0] = first_s;
                    cut_s[1] = first_u;
                }
            }
            flags[i] = flag;
        }
        carry_s += total_s;
        carry_u += total_u;
    }
    __syncthreads();                // (cut_s, whichever trip wrote it)
    const bool all = carry_s <= max_segments && carry_u <= max_units;
    const uint64_t work_s = all ? carry_s : cut_s[0], work_u = all ? carry_u : cut_s[1];
    if (tid == 0) {
        seg_prefix[count] = carry_s;
        unit_prefix[count] = carry_u;
        ctl[kSplitCtlSegments] = (uint32_t)work_s;
        ctl[kSplitCtlUnits] = (uint32_t)work_u;
        result[0] = result[1] = result[2] = result[3] = 0;
    }
    for (uint64_t k = tid; k < work_u + count; k += 1024) cuts[k] = kSplitNone;
}

// ---- 2: segment walk ----
__global__ __launch_bounds__(64) void raw_split_walk_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t segment_bytes,
                                                            const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ seg_prefix,
                                                            const uint32_t* __restrict__ flags, uint64_t* __restrict__ table,
                                                            uint4* __restrict__ nodes, uint32_t* next_segment)
{
    SNAPPY_SPLIT_WALK_SEGMENTS(items, count, segment_bytes, ctl, seg_prefix, flags, table, nodes, next_segment)
}

// ---- 3: resolve ----
__global__ __launch_bounds__(64) void raw_split_resolve_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t unit_len,
                                                               uint32_t segment_bytes, const uint64_t* __restrict__ out_len,
                                                               const uint64_t* __restrict__ seg_prefix, const uint64_t* __restrict__ unit_prefix,
                                                               uint32_t* flags, const uint64_t* __restrict__ table, uint4* __restrict__ nodes,
                                                               uint32_t* __restrict__ cuts)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t flag = uld32(reinterpret_cast<const uint8_t*>(flags + i));
        if ((flag & (kSplitClassMask | kSplitFallback)) != kSplitSplit) continue;
        SNAPPY_SPLIT_RESOLVE_CHAIN(items, i, flag, unit_len, segment_bytes, out_len, seg_prefix, table, nodes, lane)
        const uint64_t last_cut = uld64(reinterpret_cast<const uint8_t*>(unit_prefix + i)) + i + ((uint64_t)length + unit_len - 1u) / unit_len;
        if (lane == 0) {
            if (shaped) cuts[last_cut] = src_len;
            else atomicOr(flags + i, kSplitFallback);
        }
    }
}

// ---- 4: cuts ----
__global__ __launch_bounds__(64) void raw_split_cuts_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t unit_len,
                                                            const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ out_len,
                                                            const uint64_t* __restrict__ seg_prefix, const uint64_t* __restrict__ unit_prefix,
                                                            uint32_t* flags, const uint4* __restrict__ nodes, uint32_t* __restrict__ cuts,
                                                            uint32_t* next_node)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t segments = uni(ctl[kSplitCtlSegments]);

    for (;;) {
        const uint32_t p = draw_work(next_node, lane);
        if (p >= segments) break;
        const uint8_t* node = reinterpret_cast<const uint8_t*>(nodes + p);
        const uint32_t entry = uld32(node), landing = uld32(node + 4), base = uld32(node + 8);
        if (entry != kSplitNone) {
            const uint32_t i = prefix_owner<false>(seg_prefix, count, p);
            if (!(uld32(reinterpret_cast<const uint8_t*>(flags + i)) & kSplitFallback)) {
                const uint8_t* src = load_global_ptr(&items[i].src);
                const uint32_t src_len = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
                const uint32_t length = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(out_len + i));
                uint32_t* mine = cuts + (uld64(reinterpret_cast<const uint8_t*>(unit_prefix + i)) + i);
                uint32_t landed = 0, op_end;
                // (a node is step 3's own; tested all the same, so that no word of the scratch can send a load out of the stream)
                const bool ok = entry < landing && landing <= src_len && base <= length &&
                                split_walk<true>(src, src_len, entry, landing, base, length, unit_len, mine, landed, op_end);
                if ((!ok || landed != landing) && lane == 0) atomicOr(flags + i, kSplitFallback);
            }
        }
        __syncthreads();            // (the wavefront stays together from one draw to the next: see check_kernel)
    }
}

// ---- 5: unit decode ----
__global__ __launch_bounds__(64) void raw_split_units_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t unit_len,
                                                             const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ out_len,
                                                             const uint64_t* __restrict__ unit_prefix, uint32_t* flags,
                                                             const uint32_t* __restrict__ cuts, uint32_t* next_unit)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage_mem[kK2StageBytes];   // one window's output (K2's stage)
    lds_bytes_t stage = (lds_bytes_t)stage_mem;
    const uint32_t lane = threadIdx.x;
    const uint32_t all_units = uni(ctl[kSplitCtlUnits]);

    for (;;) {
        const uint32_t u = draw_work(next_unit, lane);
        if (u >= all_units) break;
        const uint32_t i = prefix_owner<false>(unit_prefix, count, u);
        const uint32_t flag = uld32(reinterpret_cast<const uint8_t*>(flags + i));
        if (!(flag & kSplitFallback)) {                              // (a mark set meanwhile and not yet seen costs time only)
            const uint8_t* src = load_global_ptr(&items[i].src);
            uint8_t* dst = load_global_ptr(&items[i].dst);
            const uint32_t src_len = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
            const uint32_t length = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(out_len + i));
            const uint32_t hdr = flag >> 8;
            const uint64_t first = uld64(reinterpret_cast<const uint8_t*>(unit_prefix + i));
            const uint32_t k = (uint32_t)(u - first);
            const uint32_t units = (uint32_t)(((uint64_t)length + unit_len - 1u) / unit_len);
            const uint8_t* cut = reinterpret_cast<const uint8_t*>(cuts + (first + i + k));
            const uint32_t a = uld32(cut), b = uld32(cut + 4);
            // the units tile [hdr, src_len): this is what the proof rests on, so it is tested here, not trusted
            const bool tiles = a != kSplitNone && b != kSplitNone && a >= hdr && a < b && b <= src_len && (k != 0 || a == hdr) &&
                               (k + 1 != units || b == src_len);
            const uint64_t at = (uint64_t)k * unit_len;
            const uint32_t left = length - (uint32_t)at;
            uint32_t st = kBlockInvalid;
            if (tiles) st = k2_decode_block<true>(src, b, a, dst + at, left < unit_len ? left : unit_len, stage);
            if (st != kBlockOk && lane == 0) atomicOr(flags + i, kSplitFallback);
        }
        __syncthreads();
    }
}

// ---- 6: serial ----
__global__ __launch_bounds__(64) void raw_split_serial_kernel(const RawItem* __restrict__ items, uint32_t count, uint64_t* __restrict__ out_len,
                                                              uint32_t* __restrict__ status, const uint32_t* __restrict__ flags,
                                                              uint32_t* result, uint32_t* next_item)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage_mem[kK2StageBytes];   // one window's output (K2's stage)
    lds_bytes_t stage = (lds_bytes_t)stage_mem;
    const uint32_t lane = threadIdx.x;

    for (;;) {
        const uint32_t i = draw_work(next_item, lane);
        if (i >= count) break;
        const uint32_t flag = uld32(reinterpret_cast<const uint8_t*>(flags + i));
        const uint32_t cls = flag & kSplitClassMask;
        if (cls == kSplitSplit && !(flag & kSplitFallback)) {         // every unit proved: out_len is the plan's
            if (lane == 0) {
                status[i] = kBlockOk;
                atomicAdd(result + 0, 1u);
            }
        } else if (cls != kSplitDone) {
            SNAPPY_RAW_DECODE_ITEM(items, i, out_len, status, stage, lane)
            if (lane == 0) atomicAdd(result + (cls == kSplitSmall ? 1 : 2), 1u);
        }
        __syncthreads();
    }
}
#endif

}  // namespace snappy_hip
