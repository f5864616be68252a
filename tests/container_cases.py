"""Framed containers for the single-call entry points (byte-range decode, byte-range overwrite): the ways a container gets
damaged, the spans asked of it, and a model of the format rules that says what the host-side front end
(csrc/dropin_plan.hpp: open_container, resolve_span, walk_to) must decide about each.  tests/test_dropin_plan.py holds the
front end to the model on the CPU; the GPU tests expect the model's status from the drop-in calls on the same bytes."""
OK, INVALID_INPUT = 0, 1


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def read_varint(data, at):
    """(value, bytes used), None where no varint32 ends within five bytes and the data."""
    v = 0
    for k in range(min(5, len(data) - at)):
        c = data[at + k]
        v |= (c & 0x7f) << (7 * k)
        if not c & 0x80:
            return v & 0xffffffff, k + 1
    return None


def read_header(stream):
    """(total, block size, header bytes) or None."""
    a = read_varint(stream, 0)
    b = read_varint(stream, a[1]) if a else None
    return (a[0], b[0], a[1] + b[1]) if b else None


def chain(stream):
    """Offsets of the size prefixes of an intact container, and its end."""
    total, bs, at = read_header(stream)
    offs = []
    for _ in range((total + bs - 1) // bs):
        offs.append(at)
        at += 4 + int.from_bytes(stream[at:at + 4], "little")
    assert at == len(stream)
    return offs + [at]


def damaged(stream):
    """kind -> bytes, the kinds of test_walker_on_goldens_and_damaged_streams and two hostile block sizes."""
    total, _, hdr = read_header(stream)
    offs = chain(stream)
    last, mid, a = offs[-2], offs[(len(offs) - 1) // 2], len(varint(total))
    return {
        "intact": stream,
        "cut in the header": stream[:hdr - 1],
        "cut in a size prefix": stream[:last + 2],
        "cut in a body": stream[:-1],
        "7 trailing bytes": stream + bytes(7),
        "a middle size field of 0x7ffffff0": stream[:mid] + (0x7ffffff0).to_bytes(4, "little") + stream[mid + 4:],
        "block size 0": stream[:a] + varint(0) + stream[hdr:],
        "block size 65536": stream[:a] + varint(65536) + stream[hdr:],
    }


HEADER_OR_CHAIN_ONLY = ("intact", "cut in the header", "cut in a size prefix", "cut in a body", "7 trailing bytes",
                        "a middle size field of 0x7ffffff0")    # (the block size stays in 1..65535: the host-mode CLI's domain)


def inner_span(bs):
    """Starts after block 0 and touches blocks 2..4."""
    return 2 * bs + 5, 2 * bs + 100


def spans(total, bs):
    s = {"first byte": (0, 1), "last byte": (total - 1, 1), "whole file": (0, total), "empty, inside": (total // 2, 0),
         "empty, at the end": (total, 0), "one byte beyond": (1, total), "wraps around": (2 ** 64 - 1, 2)}
    if total > bs:
        s["across a block boundary"] = (bs - 1, 2)
    if total > 6 * bs:
        s["blocks 2..4"] = inner_span(bs)
    return s


def model(stream, offset, length, update):
    """The rules of the format and of the two calls, in the order the calls apply them -> (status, stderr line, offsets).
    offsets: of blocks 0..upto and where the chain then stands (upto = all blocks for an update, else the last touched + 1)."""
    what = "write" if update else "range"
    h = read_header(stream)
    if not h:
        return INVALID_INPUT, "Failed to read the stream header", None
    total, bs, hdr = h
    if offset + length >= 2 ** 64 or offset + length > total:
        return INVALID_INPUT, f"snappy_hip: {what} {offset}:{length} lies beyond the {total} uncompressed bytes", None
    if not update and length == 0:
        return OK, "", []                                        # nothing to decode: the block size is never looked at
    if total and not 1 <= bs <= 65535:
        return INVALID_INPUT, f"snappy_hip: block size {bs} in the stream is outside 1..65535", None
    nb = (total + bs - 1) // bs if total else 0
    upto = nb if update else (offset + length - 1) // bs + 1
    truncated = "snappy_hip: truncated stream (block %d of %d)"
    if upto > (len(stream) - hdr) // 4:                         # every block needs its u32 size prefix
        return INVALID_INPUT, truncated % (upto - 1, nb), None
    offs, at = [], hdr
    for i in range(upto):
        if at + 4 > len(stream):
            return INVALID_INPUT, truncated % (i, nb), None
        offs.append(at)
        at += 4 + int.from_bytes(stream[at:at + 4], "little")
        if at > len(stream):                                    # block i leaves the stream: block i + 1 has no size prefix
            return INVALID_INPUT, truncated % (i + 1, nb), None
    if update and at != len(stream):
        return INVALID_INPUT, f"snappy_hip: {len(stream) - at} bytes behind the last block", None
    return OK, "", offs + [at]
