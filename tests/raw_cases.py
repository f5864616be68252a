"""Vectors of the raw Snappy batch interface (snappy_hip_raw_decompress_batch / _compress_batch), shared by the emulator and
the GPU tests.  Built by a small element writer; the expected plaintext of every intact vector comes from
tools/to_raw_snappy.decode_raw, the CPU statement of the format."""
import hashlib
import json
import os
import sys

import datagen

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import to_raw_snappy as trs   # noqa: E402

OK, INVALID, DST_TOO_SMALL, TOO_LARGE = 0, 1, 5, 6
RAW_MAX_LEN = 0x7ffff000
GUARD = 0xEE
FIXTURE_DIR = os.path.join(HERE, "golden", "raw")
FIXTURES = ["alice", "coding", "terror2", "plrabn12", "random200000", "zeros300000"]


# ---- the element writer ----
def varint(v):
    return trs.varint(v)


def literal(payload, length_bytes=None):
    """length_bytes: force a length field of 1..4 bytes (default: the shortest form)."""
    n = len(payload) - 1
    if length_bytes is None:
        if n < 60:
            return bytes([n << 2]) + payload
        length_bytes = (n.bit_length() + 7) // 8
    return bytes([(59 + length_bytes) << 2]) + n.to_bytes(length_bytes, "little") + payload


def literal_field(field, payload):
    """a literal whose 4-byte length field holds `field`, whatever the payload"""
    return bytes([63 << 2]) + field.to_bytes(4, "little") + payload


def copy1(length, offset):
    assert 4 <= length <= 11 and offset < 2048
    return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 0xff])


def copy2(length, offset):
    assert 1 <= length <= 64 and offset < 65536
    return bytes([2 | ((length - 1) << 2)]) + offset.to_bytes(2, "little")


def copy4(length, offset):
    assert 1 <= length <= 64
    return bytes([3 | ((length - 1) << 2)]) + offset.to_bytes(4, "little")


def stream(n, *elements):
    return varint(n) + b"".join(elements)


def _sized(elements):
    """the stream of these elements with the header their output needs"""
    body = b"".join(elements)
    i = 0
    n = 0
    while i < len(body):          # lengths only (the elements are the writer's own)
        tag = body[i]
        kind = tag & 3
        if kind == 0:
            ln = (tag >> 2) + 1
            i += 1
            if ln > 60:
                extra = ln - 60
                ln = int.from_bytes(body[i:i + extra], "little") + 1
                i += extra
            i += ln
        else:
            ln = ((tag >> 2) & 7) + 4 if kind == 1 else (tag >> 2) + 1
            i += {1: 2, 2: 3, 3: 5}[kind]
        n += ln
    return varint(n) + body


# ---- intact vectors: name -> stream ----
def intact_vectors():
    v = {}
    r = datagen.random_bytes
    v["literal_65537"] = _sized([literal(r(65537, seed=11))])
    v["literal_300000"] = _sized([literal(r(300000, seed=12))])
    # 120,000 bytes of literal, then copies that reach back further than any block of the framed format is long
    v["copy4_far"] = _sized([literal(r(120000, seed=13))] + [copy4(64 - k % 7, 65536 + 977 * k) for k in range(40)] + [copy4(5, 119999)])
    v["copy2_65535"] = _sized([literal(r(65535, seed=14))] + [copy2(64, 65535), copy2(1, 65535), copy2(33, 65535)])
    # overlapping copies (offsets 1..7) laid across the 64 KiB boundary of the output
    v["overlap_64k"] = _sized([literal(r(65536 - 100, seed=15))] + [copy1(11, off) for off in range(1, 8)] * 6 + [copy2(64, off) for off in range(1, 8)])
    v["empty"] = stream(0)
    v["one_byte"] = _sized([literal(b"x")])
    # headers of 1..5 bytes: the shortest forms of 1 .. 3 bytes, then padded forms (more bytes than the value needs)
    v["header_1"] = _sized([literal(r(100, seed=16))])
    v["header_2"] = _sized([literal(r(200, seed=17))])
    v["header_3"] = _sized([literal(r(20000, seed=18))])
    v["header_4_padded"] = bytes([0x80 | 100, 0x80, 0x80, 0x00]) + literal(r(100, seed=19))
    v["header_5_padded"] = bytes([0x80 | 100, 0x80, 0x80, 0x80, 0x00]) + literal(r(100, seed=20))
    v["all_types"] = _sized([literal(r(3000, seed=21)), copy1(7, 2047), copy2(64, 3000), copy4(17, 2999), literal(b"tail" * 20, 3),
                             copy1(4, 1), literal(r(61, seed=22), 4), copy4(64, 64)])
    return v


# ---- damaged vectors: name -> stream; every one is BLOCK_INVALID ----
def damaged_vectors():
    v = {}
    r = datagen.random_bytes
    lit = literal(r(500, seed=31))
    v["offset_0"] = stream(510, lit, copy2(10, 0))
    v["offset_beyond_output"] = stream(510, lit, copy2(10, 501))
    v["offset_beyond_output_copy4"] = stream(510, lit, copy4(10, 0x80000000))
    for field in (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFF00):
        v["literal_field_%08X" % field] = stream(600, literal(r(100, seed=32)), literal_field(field, r(300, seed=33)))
        v["literal_field_%08X_first" % field] = stream(40, literal_field(field, r(40, seed=34)))
    v["output_one_more"] = stream(500, literal(r(501, seed=35)))
    v["output_one_more_copy"] = stream(509, lit, copy2(10, 7))
    v["output_one_less"] = stream(501, lit)
    v["trailing_byte"] = stream(500, lit) + b"\x00"
    v["trailing_element"] = stream(500, lit, copy2(4, 4))
    whole = stream(1510, literal(r(1000, seed=36)), copy2(10, 500), literal(r(500, seed=37), 4))
    v["cut_inside_tag"] = whole[:2 + 3 + 1000 + 1]                     # the copy's tag without its offset bytes
    v["cut_inside_length_field"] = whole[:2 + 3 + 1000 + 3 + 3]         # the second literal's tag and two of its four length bytes
    v["cut_inside_payload"] = whole[:-1]
    v["cut_inside_first_payload"] = whole[:700]
    v["header_fifth_byte_16"] = bytes([0x80, 0x80, 0x80, 0x80, 0x10]) + literal(b"x")
    v["header_6_bytes"] = bytes([0x80 | 1, 0x80, 0x80, 0x80, 0x80, 0x00]) + literal(b"x")
    v["header_unfinished"] = bytes([0x80, 0x80])
    v["no_bytes"] = b""
    v["empty_with_trailing"] = stream(0) + literal(b"x")
    return v


def header_parses(s):
    """(length, header bytes) as Google's decoder reads a varint32, or None"""
    v = 0
    for k in range(min(5, len(s))):
        c = s[k]
        if k == 4 and c >= 16:
            return None
        v |= (c & 0x7f) << (7 * k)
        if c < 0x80:
            return v, k + 1
    return None


def expect(s, capacity=None):
    """-> (status, out_len, plaintext or None) of one item with `capacity` bytes at dst (None: exactly the header's length)"""
    h = header_parses(s)
    if h is None:
        return INVALID, 0, None
    n = h[0]
    if len(s) > RAW_MAX_LEN or n > RAW_MAX_LEN:
        return TOO_LARGE, n, None
    if capacity is not None and n > capacity:
        return DST_TOO_SMALL, n, None
    try:
        plain = trs.decode_raw(s)
    except (ValueError, IndexError):
        return INVALID, n, None
    return OK, n, plain


# ---- fixtures: third-party streams (pyarrow's Snappy codec = Google's), tools/record_raw_fixtures.py ----
def fixture_plain(name):
    if name == "random200000":
        return datagen.random_bytes(200000, seed=7)
    if name == "zeros300000":
        return datagen.zeros(300000)
    with open(os.path.join(HERE, "golden", name + ".txt"), "rb") as f:
        return f.read()


def fixture_stream(name):
    with open(os.path.join(FIXTURE_DIR, name + ".raw_snappy"), "rb") as f:
        s = f.read()
    with open(os.path.join(FIXTURE_DIR, "fixtures.json")) as f:
        meta = json.load(f)[name]
    assert len(s) == meta["stream_len"] and hashlib.sha256(s).hexdigest() == meta["stream_sha256"], name
    return s


# ---- compress: item lengths around a fragment ----
def compress_lengths(block_size):
    return sorted({0, 1, 63, 64, block_size - 1, block_size, block_size + 1, 2 * block_size + block_size // 3})
