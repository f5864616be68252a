// dropin_plan.hpp -- where the drop-in pair (csrc/dropin_pair.hpp) puts every byte.  Plain C++, no HIP, no environment
// reads (the caller passes the knobs): tests/test_dropin_plan.py compiles it on the CPU.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/snappy_hip.h"
#include "host_chain.hpp"

namespace dropin_plan {

using host_chain::le32;

// a shard of the file, or a chunk of a shard (then relative to the shard): blocks and their plaintext slice
struct Range {
    uint64_t first_block = 0, num_blocks = 0;
    uint64_t plain_off = 0, plain_len = 0;
};

// `count` ranges of `per` blocks out of nb blocks (plain_len bytes); the last non-empty one may be shorter
inline std::vector<Range> cut(uint64_t nb, uint64_t per, uint64_t count, uint64_t plain_len, uint32_t bs)
{
    std::vector<Range> v(count);
    for (uint64_t k = 0; k < count; ++k) {
        Range& r = v[k];
        r.first_block = std::min(nb, k * per);
        r.num_blocks = std::min(nb, r.first_block + per) - r.first_block;
        if (!r.num_blocks) continue;
        r.plain_off = r.first_block * bs;
        r.plain_len = std::min(plain_len - r.plain_off, r.num_blocks * bs);
    }
    return v;
}

// shards used for a file of nb blocks: no more than there are blocks, and one for an empty file (it does nothing)
inline int shard_count(int want, uint64_t nb) { return (uint64_t)want > nb ? (nb ? (int)nb : 1) : want; }
inline uint64_t shard_blocks(uint64_t nb, int shards) { return (nb + shards - 1) / shards; }

// contiguous ranges of ceil(nb / shards) blocks (snappy_compress.c:494-520)
inline std::vector<Range> partition(uint64_t nb, int shards, uint64_t total_len, uint32_t bs)
{
    return cut(nb, shard_blocks(nb, shards), shards, total_len, bs);
}

// Blocks per pipeline chunk.  knob = SNAPPY_HIP_PIPELINE_BLOCKS (null: unset; 0 = strictly phased).  Default: 128 MiB
// (4096 blocks of 32 KiB: one block per resident wavefront), shrinking to a quarter of the shard but not below 64 MiB, so
// that a 256 MiB file still overlaps; sized in bytes, since small blocks would make the pipeline bound by launches.
inline uint64_t pipeline_chunk_blocks(uint64_t shard_blocks, uint32_t block_size, const char* knob)
{
    if (knob && *knob) return atoi(knob) > 0 ? (uint64_t)atoi(knob) : 0;
    const uint64_t scale = std::max<uint64_t>(1, 32768 / std::max<uint32_t>(block_size, 1));
    const uint64_t quarter = ((shard_blocks + 3) / 4 + 15) & ~15ull;
    return std::min<uint64_t>(4096 * scale, std::max<uint64_t>(2048 * scale, quarter));
}

// compress: chunks of `chunk` blocks when the shard is longer than one, else one chunk per shard (the phased form)
inline uint64_t compress_chunk_blocks(uint64_t per, uint64_t chunk)
{
    return (!chunk || per <= chunk) ? std::max<uint64_t>(per, 1) : chunk;
}

// decompress: a decode launch costs about the same for 2048 blocks as for 8192, so overlapping pays from three chunks per
// shard.  One overlapped shard walks the size chain inside its pipeline; otherwise it is walked up front.
struct DecompressChunking { uint64_t chunk_blocks; bool walk_in_pipeline; };
inline DecompressChunking decompress_chunking(uint64_t per, uint64_t chunk, int shards)
{
    const bool overlapped = chunk && per >= 3 * chunk;
    return {overlapped ? chunk : std::max<uint64_t>(per, 1), overlapped && shards == 1};
}

// equal chunks of at most `chunk` (> 0) blocks, each a multiple of 16 blocks: 16-byte aligned slices whatever the block size
inline std::vector<Range> split_blocks(uint64_t nb, uint64_t plain_len, uint32_t bs, uint64_t chunk)
{
    if (!nb) return {};
    const uint64_t parts = (nb + chunk - 1) / chunk;
    const uint64_t per = ((nb + parts - 1) / parts + 15) & ~15ull;
    return cut(nb, per, (nb + per - 1) / per, plain_len, bs);
}

inline uint32_t put_varint32(uint8_t* dst, uint32_t v)   // snappy_compress.c:69-98
{
    uint32_t k = 0;
    while (v >= 0x80) {
        dst[k++] = (uint8_t)(v | 0x80);
        v >>= 7;
    }
    dst[k++] = (uint8_t)v;
    return k;
}
inline uint32_t get_varint32(const uint8_t* src, uint64_t avail, uint32_t* out)   // snappy_decompress.c:23-37; 0 = unreadable
{
    uint32_t v = 0;
    for (uint32_t k = 0; k < 5 && k < avail; ++k) {
        const uint8_t c = src[k];
        v |= (uint32_t)(c & 0x7f) << (7 * k);
        if (!(c & 0x80)) {
            *out = v;
            return k + 1;
        }
    }
    return 0;
}
inline uint32_t varint32_len(uint32_t v)   // bytes of put_varint32
{
    uint32_t k = 1;
    for (; v >= 0x80; v >>= 7) ++k;
    return k;
}
inline uint64_t pad256(uint64_t v) { return (v + 255) & ~255ull; }

// a compress chunk frames its blocks as a stream of its own in the stream pool (the host drops its local header)
struct CompressChunk : Range {
    uint32_t local_hdr = 0;                     // header bytes of snappy_hip_write_header(plain_len, bs)
    uint64_t stream_at = 0, offsets_at = 0;     // byte offsets into the two pools, 256-byte aligned
};
struct CompressLayout { std::vector<CompressChunk> chunks; uint64_t stream_pool = 0, offsets_pool = 0; };

// stride = snappy_hip_slot_stride(bs), so that 10 + blocks * stride = snappy_hip_stream_bound of a chunk
inline CompressLayout compress_layout(uint64_t nb, uint64_t plain_len, uint32_t bs, uint32_t stride, uint64_t chunk)
{
    CompressLayout l;
    for (const Range& r : split_blocks(nb, plain_len, bs, chunk)) {
        CompressChunk c;
        static_cast<Range&>(c) = r;
        c.local_hdr = varint32_len((uint32_t)c.plain_len) + varint32_len(bs);
        c.stream_at = l.stream_pool;
        c.offsets_at = l.offsets_pool;
        l.stream_pool += pad256(10 + c.num_blocks * stride);
        l.offsets_pool += pad256((c.num_blocks + 1) * sizeof(uint64_t));
        l.chunks.push_back(c);
    }
    return l;
}

// The serial walk of the size chain (snappy_decompress.c:317-340) from block `block` at stream position `at` on to block
// `upto`: rel[i] = (start of block i) - base for every block passed, and rel[block] where it then stands.  It stops at a
// block whose u32 size prefix is not in buf[0, len) (kTruncated) or which ends beyond it (kLeaves; `at` = that end).
enum Stop { kDone, kTruncated, kLeaves };
struct Walk { uint64_t block = 0, at = 0; Stop stop = kDone; };
inline Walk walk_chain(const uint8_t* buf, uint64_t len, uint64_t base, uint64_t* rel, Walk w, uint64_t upto)
{
    for (; w.block < upto; ++w.block) {
        if (w.at + 4 > len) return {w.block, w.at, kTruncated};
        rel[w.block] = w.at - base;
        w.at += 4 + (uint64_t)le32(buf + w.at);
        if (w.at > len) return {w.block, w.at, kLeaves};
    }
    rel[w.block] = w.at - base;
    return {w.block, w.at, kDone};
}

// the verdict on a walk of all nb blocks of a stream of len bytes: empty if the chain ends exactly at the stream's end;
// else the first block whose size prefix is not in the stream (the one after a block that leaves it), or where it ends
inline std::string whole_walk_error(const Walk& w, uint64_t nb, uint64_t len)
{
    const uint64_t cut = w.stop == kLeaves ? w.block + 1 : w.block;
    char m[96] = "";
    if (w.stop != kDone && cut < nb)
        snprintf(m, sizeof m, "truncated stream (block %lu of %lu)", (unsigned long)cut, (unsigned long)nb);
    else if (w.at != len)
        snprintf(m, sizeof m, "size chain ends at %lu, stream has %lu bytes", (unsigned long)w.at, (unsigned long)len);
    return m;
}

// ---- The front end of the single-device calls on one framed file (byte-range decode, byte-range overwrite): what the host
// decides about an untrusted container before anything is sized by it or sent to a device. ----

inline bool block_size_ok(uint32_t bs) { return bs >= SNAPPY_HIP_MIN_BLOCK_SIZE && bs <= SNAPPY_HIP_MAX_BLOCK_SIZE; }

// What a check decided: the status for the caller and the line for stderr (this file prints nothing).
struct Verdict {
    snappy_status status = SNAPPY_OK;
    std::string message;
    explicit operator bool() const { return status != SNAPPY_OK; }
};
__attribute__((format(printf, 1, 2))) inline Verdict refuse(const char* fmt, ...)
{
    char m[160] = "snappy_hip: ";
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(m + 12, sizeof m - 12, fmt, ap);
    va_end(ap);
    return {SNAPPY_INVALID_INPUT, m};
}
inline Verdict unreadable_header() { return {SNAPPY_INVALID_INPUT, "Failed to read the stream header"}; }   // the reference's words
inline Verdict bad_block_size(uint32_t bs, const char* where) { return refuse("block size %u%s is outside 1..65535", bs, where); }

// the two varints in front of the first block (snappy_decompress.c:193-198, :298-303); 0 = unreadable
inline uint32_t parse_header(const uint8_t* buf, uint64_t len, uint32_t* total, uint32_t* bs)
{
    const uint32_t a = get_varint32(buf, len, total);
    const uint32_t b = a ? get_varint32(buf + a, len - a, bs) : 0;
    return b ? a + b : 0;
}

// A framed file: header bytes, uncompressed bytes, block size, blocks.  `bad` = the header cannot be read (hdr = 0), or the
// file has bytes and its block size is outside 1..65535 (hdr != 0, nb = 0).  The functions below return it where it first
// matters to them: resolve_span an unreadable header, walk_to either -- so a span beyond the file is refused as such, and
// an empty range served, whatever the block size says.
struct Container {
    uint32_t hdr = 0, total = 0, bs = 0;
    uint64_t nb = 0;
    Verdict bad;
};
inline Container open_container(const uint8_t* buf, uint64_t len)
{
    Container c;
    c.hdr = parse_header(buf, len, &c.total, &c.bs);
    if (!c.hdr)
        c.bad = unreadable_header();
    else if (c.total && !block_size_ok(c.bs))
        c.bad = bad_block_size(c.bs, " in the stream");
    else if (c.total)
        c.nb = ((uint64_t)c.total + c.bs - 1) / c.bs;
    return c;
}

// the blocks that plaintext bytes [offset, offset + length) touch: none for an empty span (or while c.bad)
struct Span { uint64_t first = 0, last = 0, blocks = 0; };
inline Verdict resolve_span(const Container& c, uint64_t offset, uint64_t length, const char* what, Span* s)
{
    *s = Span{};
    if (!c.hdr) return c.bad;
    if (offset + length < offset || offset + length > c.total)
        return refuse("%s %lu:%lu lies beyond the %u uncompressed bytes", what, (unsigned long)offset, (unsigned long)length, c.total);
    if (length && c.nb) *s = {offset / c.bs, (offset + length - 1) / c.bs, (offset + length - 1) / c.bs - offset / c.bs + 1};
    return {};
}

// The size chain from the header up to block `upto`: off[i] = stream offset of block i for i < upto, off[upto] = where the chain
// then stands.  Every block needs its u32 size prefix, which is checked before anything is sized by the header-derived
// count.  A walk that stops names the first block whose prefix is not in the stream (the one after a block that leaves it).
// to_the_end: the chain must end exactly where the stream does.
inline Verdict walk_to(const uint8_t* buf, uint64_t len, const Container& c, uint64_t upto, bool to_the_end, std::vector<uint64_t>& off)
{
    if (c.bad) return c.bad;
    if (upto > (len - c.hdr) / 4) return refuse("truncated stream (block %lu of %lu)", (unsigned long)(upto - 1), (unsigned long)c.nb);
    off.assign(upto + 1, 0);
    const Walk w = walk_chain(buf, len, 0, off.data(), {0, c.hdr}, upto);
    if (w.stop != kDone)
        return refuse("truncated stream (block %lu of %lu)", (unsigned long)(w.stop == kLeaves ? w.block + 1 : w.block), (unsigned long)c.nb);
    if (to_the_end && w.at != len) return refuse("%lu bytes behind the last block", (unsigned long)(len - w.at));
    return {};
}

}  // namespace dropin_plan
