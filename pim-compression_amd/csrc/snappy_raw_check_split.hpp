// snappy_raw_check_split.hpp -- ONE large raw Snappy stream CHECKED by many wavefronts, whatever its shape
// (snappy_hip_raw_check_split_batch, include/snappy_hip.h).
//
// raw_check_kernel (snappy_check.hpp) gives a whole stream to one wavefront.  The split decode (snappy_raw_split.hpp) spreads a
// stream over the device only where it is built from independent fragments, because a copy needs the output in front of it.  A
// check needs no output: every test k2_check_block<true> makes uses an element's own fields and its ABSOLUTE output position --
// an element predecode rejects, output beyond the header's length, a copy whose offset is 0 or larger than its output
// position, and a chain that does not end exactly at src_len with exactly `length` bytes.  Steps 2 and 3 of the split decode
// already give every stretch of the true chain its (entry, landing, output base); so any stream can be checked segment by
// segment: no unit, no cuts, no assumption about fragments.
//
// One phased call, each step a kernel (those of this file are compiled by snappy_hip_raw_check_split.hip, the library's second
// source, which takes the __device__ pieces of the other headers without their kernels: SNAPPY_HIP_NO_KERNELS):
//   1 raw_vsplit_plan_kernel     one workgroup: the header rules of raw_check_kernel (SNAPPY_RAW_ITEM_VERDICT without its capacity
//                                rule), out_len and the header-level verdicts; an item is LARGE when its elements span more than
//                                one segment; the exclusive prefix of the large items' segments; the first large item that does
//                                not fit max_segments and every large one behind it go to the serial checker.
//   2 raw_vsplit_walk_kernel     the split decode's step 2, the same text (SNAPPY_SPLIT_WALK_SEGMENTS): 64 candidate chains per
//                                segment, sizes only.
//   3 raw_vsplit_resolve_kernel  the split decode's step 3 without its cuts (SNAPPY_SPLIT_RESOLVE_CHAIN): one wavefront per item,
//                                one node (entry, landing, output base) per step of the true chain; an item is "shaped" iff the
//                                chain ends exactly at src_len with the header's length as its sum; the others are marked.
//   4 raw_vsplit_verify_kernel   persistent wavefronts, one node each: the node's elements are walked by split_walk in its
//                                kOffsets mode from `entry` with the output position `base`.  The item is marked when an element
//                                is rejected, the output passes `length`, a copy's offset is 0 or larger than base + its position
//                                in the node, the walk does not land where the node says, or the node does not LINK: the walk's
//                                output must end at the base of the node that starts at its landing (at `length` when the
//                                landing is src_len), and the node of an item's first segment must start at the header's end
//                                with base 0.  No LDS, no payload loaded, no store but the mark.
//   5 raw_vsplit_serial_kernel   raw_check_kernel's trip (SNAPPY_RAW_CHECK_ITEM) over the items that are not large and the marked
//                                ones; large items that are shaped and unmarked get SNAPPY_HIP_BLOCK_OK and the plan's length.
//                                Counts the three classes into d_result.
//
// WHY IT IS EXACT.  A large item gets OK from steps 1-4 only if (a) step 3 followed nodes from the header's end to src_len, and
// (b) step 4 left every one of its nodes unmarked.  By (b) and induction along the links -- the first node starts at the
// header's end at output position 0, every node's walk starts at an element start with its true output position and ends, with
// the true output sum, exactly where the next node starts -- the nodes' elements, in order, ARE the item's element stream, it
// ends exactly at src_len with exactly `length` bytes, and every element on it passed predecode_window<true>'s tests, the
// length bound and the offset test at its absolute position: the serial checker's tests on the same elements, so its verdict
// is OK and its length the header's.  Every other large item -- unshaped, marked, or beyond max_segments -- and every item
// that is not large is judged by the serial checker itself in step 5.  So (status, out_len) is always what
// snappy_hip_raw_check_batch gives; a mistake in steps 2-4 can cost time and never a verdict.  Conversely a VALID large item
// inside the limits is never marked: its true chain is shaped, and its elements pass every test at their true positions.
// All cursors are 32 bits wide under kRawMaxLen, as in snappy_raw_split.hpp.
#pragma once
#include "snappy_device_common.hpp"
#include "snappy_kernels.hpp"     // window_issue, predecode_window, k2_chain_walk
#include "snappy_raw.hpp"         // RawItem, kRawMaxLen, SNAPPY_RAW_ITEM_VERDICT
#include "snappy_check.hpp"       // k2_check_block, SNAPPY_RAW_CHECK_ITEM
#include "snappy_raw_split.hpp"   // split_element_size, split_walk, the flag words, the walk's and the resolve's text

namespace snappy_hip {

// Scratch of one call, every part rounded up to 256 bytes: control line (kSplitCtlSegments), seg_prefix[count + 1] (u64: first
// segment of item i among the large items'), flags[count] (the split decode's flag words: class, "check it serially", the
// header's length), table[max_segments][64] (u64: landing | output bytes << 32) and nodes[max_segments] (uint4: entry, landing,
// output base; the node of a step lives at the segment of its entry).
struct VsplitLayout {
    uint64_t seg_prefix, flags, table, nodes, total;
};
__host__ __device__ inline VsplitLayout vsplit_layout(uint32_t count, uint64_t max_segments)
{
    if (max_segments > kSplitMaxWork) max_segments = kSplitMaxWork;
    VsplitLayout l;
    l.seg_prefix = 256;
    l.flags = l.seg_prefix + round256(((uint64_t)count + 1u) * 8u);
    l.table = l.flags + round256((uint64_t)count * 4u);
    l.nodes = l.table + round256(max_segments * kSplitZone * 8u);
    l.total = l.nodes + round256(max_segments * 16u);
    return l;
}

// ---- 1: plan ----
__global__ __launch_bounds__(1024) void raw_vsplit_plan_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t segment_bytes,
                                                               uint64_t max_segments, uint64_t* __restrict__ out_len,
                                                               uint32_t* __restrict__ status, uint32_t* __restrict__ result,
                                                               uint32_t* __restrict__ ctl, uint64_t* __restrict__ seg_prefix,
                                                               uint32_t* __restrict__ flags)
{
    __shared__ uint64_t wave_sums[16];
    __shared__ uint64_t cut_s;      // segments in front of the first item beyond the limit
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < count; base += 1024) {
        const uint32_t i = base + tid;
        uint64_t segs = 0;
        uint32_t flag = kSplitDone;
        if (i < count) {
            SNAPPY_RAW_ITEM_VERDICT(items, i, ld64, uint32_t, kSplitPending)
            (void)dst;
            // a check has no capacity rule: the two verdicts that stand behind it in SNAPPY_RAW_ITEM_VERDICT
            if (st == kRawDstTooSmall) st = length == 0 ? (src_len == hdr ? kBlockOk : kBlockInvalid) : kSplitPending;
            out_len[i] = length;
            if (st != kSplitPending) {
                status[i] = st;
            } else {
                const uint64_t s = (src_len - hdr + segment_bytes - 1u) / segment_bytes;
                flag = kSplitSmall | (hdr << 8);
                if (s > 1) {
                    flag = kSplitSplit | (hdr << 8);
                    segs = s;
                }
            }
        }
        uint64_t total;
        const uint64_t first = carry + workgroup_exclusive_scan(segs, wave_sums, total);
        if (i < count) {
            seg_prefix[i] = first;
            // past the limit: the first such item (exactly one starts inside it) marks the end of the work
            if (segs && first + segs > max_segments) {
                flag |= kSplitFallback;
                if (first <= max_segments) cut_s = first;
            }
            flags[i] = flag;
        }
        carry += total;
    }
    __syncthreads();                // (cut_s, whichever trip wrote it)
    if (tid == 0) {
        seg_prefix[count] = carry;
        ctl[kSplitCtlSegments] = (uint32_t)(carry <= max_segments ? carry : cut_s);
        result[0] = result[1] = result[2] = result[3] = 0;
    }
}

// ---- 2: segment walk ----
__global__ __launch_bounds__(64) void raw_vsplit_walk_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t segment_bytes,
                                                             const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ seg_prefix,
                                                             const uint32_t* __restrict__ flags, uint64_t* __restrict__ table,
                                                             uint4* __restrict__ nodes, uint32_t* next_segment)
{
    SNAPPY_SPLIT_WALK_SEGMENTS(items, count, segment_bytes, ctl, seg_prefix, flags, table, nodes, next_segment)
}

// ---- 3: resolve ----
__global__ __launch_bounds__(64) void raw_vsplit_resolve_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t segment_bytes,
                                                                const uint64_t* __restrict__ out_len, const uint64_t* __restrict__ seg_prefix,
                                                                uint32_t* flags, const uint64_t* __restrict__ table, uint4* __restrict__ nodes)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t flag = uld32(reinterpret_cast<const uint8_t*>(flags + i));
        if ((flag & (kSplitClassMask | kSplitFallback)) != kSplitSplit) continue;
        SNAPPY_SPLIT_RESOLVE_CHAIN(items, i, flag, 0u, segment_bytes, out_len, seg_prefix, table, nodes, lane)
        if (!shaped && lane == 0) atomicOr(flags + i, kSplitFallback);
    }
}

// ---- 4: verify ----
__global__ __launch_bounds__(64) void raw_vsplit_verify_kernel(const RawItem* __restrict__ items, uint32_t count, uint32_t segment_bytes,
                                                               const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ out_len,
                                                               const uint64_t* __restrict__ seg_prefix, uint32_t* flags,
                                                               const uint4* __restrict__ nodes, uint32_t* next_node)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t segments = uni(ctl[kSplitCtlSegments]);

    for (;;) {
        const uint32_t p = draw_work(next_node, lane);
        if (p >= segments) break;
        const uint8_t* node = reinterpret_cast<const uint8_t*>(nodes + p);
        const uint32_t entry = uld32(node), landing = uld32(node + 4), base = uld32(node + 8);
        const uint32_t i = prefix_owner<false>(seg_prefix, count, p);
        const uint32_t flag = uld32(reinterpret_cast<const uint8_t*>(flags + i));
        const uint64_t first = uld64(reinterpret_cast<const uint8_t*>(seg_prefix + i));
        const uint32_t hdr = flag >> 8;
        if (!(flag & kSplitFallback)) {                              // (a mark set meanwhile and not yet seen costs time only)
            bool ok;
            if (entry == kSplitNone) {
                ok = p != first;                                     // the chain passes this segment by; never an item's first
            } else {
                const uint8_t* src = load_global_ptr(&items[i].src);
                const uint32_t src_len = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(&items[i].src_len));
                const uint32_t length = (uint32_t)uld64(reinterpret_cast<const uint8_t*>(out_len + i));
                // (a node is step 3's own; tested all the same, so that no word of the scratch can send a load out of the stream
                // or out of the item's nodes)
                ok = entry >= hdr && entry < landing && landing <= src_len && base <= length && (p != first || (entry == hdr && base == 0));
                uint32_t want_end = length;
                if (ok && landing < src_len) {                       // the link: the node that starts where this one lands
                    const uint8_t* next = reinterpret_cast<const uint8_t*>(nodes + (first + (landing - hdr) / segment_bytes));
                    ok = uld32(next) == landing;
                    want_end = uld32(next + 8);
                }
                uint32_t landed = 0, op_end = 0;
                ok = ok && split_walk<false, true>(src, src_len, entry, landing, base, length, 0u, nullptr, landed, op_end) && landed == landing &&
                     op_end == want_end;
            }
            if (!ok && lane == 0) atomicOr(flags + i, kSplitFallback);
        }
        __syncthreads();            // (the wavefront stays together from one draw to the next: see check_kernel)
    }
}

// ---- 5: serial ----
__global__ __launch_bounds__(64) void raw_vsplit_serial_kernel(const RawItem* __restrict__ items, uint32_t count, uint64_t* __restrict__ out_len,
                                                               uint32_t* __restrict__ status, const uint32_t* __restrict__ flags,
                                                               uint32_t* result, uint32_t* next_item)
{
    const uint32_t lane = threadIdx.x;

    for (;;) {
        const uint32_t i = draw_work(next_item, lane);
        if (i >= count) break;
        const uint32_t flag = uld32(reinterpret_cast<const uint8_t*>(flags + i));
        const uint32_t cls = flag & kSplitClassMask;
        if (cls == kSplitSplit && !(flag & kSplitFallback)) {         // every node proved: out_len is the plan's
            if (lane == 0) {
                status[i] = kBlockOk;
                atomicAdd(result + 0, 1u);
            }
        } else if (cls != kSplitDone) {
            SNAPPY_RAW_CHECK_ITEM(items, i, out_len, status, lane)
            if (lane == 0) atomicAdd(result + (cls == kSplitSmall ? 1 : 2), 1u);
        }
        __syncthreads();
    }
}

}  // namespace snappy_hip
