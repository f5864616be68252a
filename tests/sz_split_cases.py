"""Seeded cases of the split walk of .sz streams (snappy_hip_sz_decompress_split_batch), shared by the emulator and the GPU
tests, built over tests/sz_cases.py: its writers, its damaged streams and its strict reader, which is the yardstick.  Also the
plain-Python statement of which large items the parallel walk proves -- those whose chain parses and whose segments lie inside
max_segments -- which makes d_result[2] and d_result[3] exact expectations.

The shapes are the smallest that can go wrong: streams of 4 - 64 KiB, chunks of 64 - 4096 bytes, segments of 256 - 4096 bytes."""
import functools

import datagen
import raw_cases as rc
import sz_cases as sz

ID = sz.IDENTIFIER


class Case:
    """One batch.  items: (label, stream, capacity, item flags, src_len); path: the labels of the model-writer items whose chunks
    are at most half a segment long (three quarters of their segments must lie on the proven path)."""

    def __init__(self, name, segment_bytes, max_chunks=4096, max_segments=None, flags=0):
        self.name, self.segment_bytes, self.max_chunks, self.flags = name, segment_bytes, max_chunks, flags
        self.max_segments_given = max_segments
        self.items, self.path = [], []

    def add(self, label, stream, capacity=None, item_flags=0, src_len=None, slack=0, path=False):
        if capacity is None:
            capacity = sz.read_sz(stream)[1] + slack
        self.items.append((label, stream, capacity, item_flags, len(stream) if src_len is None else src_len))
        if path:
            self.path.append(label)
        return self

    @property
    def batch(self):
        """the items as the emulator's and the GPU tests' Batch classes take them"""
        return [(s, cap, fl, n) for _, s, cap, fl, n in self.items]

    @property
    def max_segments(self):
        if self.max_segments_given is not None:
            return self.max_segments_given
        return sum(segments(n, self.segment_bytes) for _, _, _, _, n in self.items)


def segments(src_len, segment_bytes):
    return -(-src_len // segment_bytes)


# ---- the model: which large items does the parallel walk prove? ----
def chain_parses(stream):
    st, _, _, bad = sz.read_sz(stream, verify=False)
    return st not in (sz.INVALID, sz.UNSUPPORTED) or bad != sz.NONE


def expected_split_result(case):
    """-> (d_result[2], d_result[3]): large items proven / walked serially.  Large: more than one segment, and not settled before
    any walk (a null src, src_len above the maximum).  The segments of the large items are counted in item order; an item that
    ends beyond max_segments, and so every large one behind it, is walked serially; so is one whose chain does not parse."""
    proven = serial = first = 0
    for _, s, _, fl, n in case.items:
        if (fl & 1) or n > rc.RAW_MAX_LEN or n <= case.segment_bytes:
            continue
        segs = segments(n, case.segment_bytes)
        inside = first + segs <= case.max_segments
        first += segs
        if inside and chain_parses(s[:n]):
            proven += 1
        else:
            serial += 1
    return proven, serial


# ---- stream pieces ----
def mix(n, seed):
    return sz.text_random_mix(n, seed)


def data_chunks(plain, chunk_len):
    """the model writer's data chunks over the oracle's blocks, without the identifier"""
    return sz.write_sz_oracle(plain, chunk_len)[len(ID):]


def pad_to(stream, n):
    """a padding chunk that brings the stream to exactly n bytes"""
    assert n - len(stream) >= 4
    return stream + sz.chunk(0xfe, bytes(n - len(stream) - 4))


@functools.lru_cache(maxsize=None)
def filler(seed, n=5000, chunk_len=300):
    """valid data chunks of about n plain bytes"""
    return data_chunks(mix(n, seed), chunk_len)


# ---- geometry ----
@functools.lru_cache(maxsize=None)
def geometry_cases():
    out = []
    seg = 1024
    c = Case("geometry_1024", seg)
    c.add("small in front", sz.intact_streams()["padding_and_skippable"][0], slack=3)
    body = ID + filler(1, 900, 150)
    assert len(body) < seg - 4
    c.add("src_len == segment_bytes", pad_to(body, seg))
    c.add("src_len == segment_bytes + 1", pad_to(body, seg + 1), slack=5)
    c.add("an exact multiple", pad_to(ID + filler(2, 6000, 250), 8 * seg))
    # chunk boundaries exactly at a share's first byte, at least five data chunks behind each
    s = ID
    for k in range(1, 5):
        s = pad_to(s + filler(10 + k, 200, 100), k * seg) + filler(20 + k, 700, 100)
        assert len(s) < (k + 1) * seg - 4
    c.add("boundaries at share starts", s)
    rnd = datagen.random_bytes(16384 + 100, seed=40)
    c.add("no boundary in most shares", sz.write_sz_oracle(rnd, 4096), slack=1)
    c.add("one chunk", ID + sz.data_chunk(rnd[:4096]))
    c.add("writer chunks of 256", sz.write_sz_oracle(mix(20000, 41), 256), path=True)
    c.add("pyarrow chunks of 480", sz.write_sz_pyarrow(mix(12000, 42), 480), path=True)
    c.add("damaged small behind", sz.damaged_streams()["reserved_unskippable_02"])
    out.append(c)
    c = Case("geometry_256", 256)
    c.add("no boundary in any share but one in 16", sz.write_sz_oracle(rnd[:12288], 4096))
    c.add("writer chunks of 64", sz.write_sz_oracle(mix(6000, 43), 64), path=True)
    c.add("src_len 257", pad_to(ID + filler(3, 200, 100), 257))
    c.add("one chunk", ID + sz.data_chunk(rnd[:1000]), slack=2)
    out.append(c)
    c = Case("geometry_4096", 4096)
    c.add("writer chunks of 2000", sz.write_sz_oracle(mix(60000, 44), 2000), path=True)
    c.add("pyarrow chunks of 1000", sz.write_sz_pyarrow(mix(30000, 45), 1000), path=True)
    c.add("incompressible chunks of 4096", sz.write_sz_oracle(rnd, 4096))
    out.append(c)
    return out


# ---- chain contents and decoys ----
@functools.lru_cache(maxsize=None)
def content_cases():
    seg = 512
    c = Case("contents_512", seg)
    a, b = mix(7000, 50), mix(6000, 51)
    c.add("identifier repeated", sz.write_sz_oracle(a, 300) + sz.write_sz_oracle(b, 200) + ID + ID + filler(52, 2000, 100))
    s = ID
    for k in range(6):
        s += filler(60 + k, 900, 150) + sz.chunk(0x80 if k % 2 else 0xfe, bytes([k]) * (7 * k))
    s += sz.chunk(0x80, datagen.random_bytes(3000, seed=61)) + filler(62, 2500, 120) + sz.chunk(0xfd, b"")
    c.add("skippable chunks, one over several shares", s)
    s = ID + filler(70, 1500, 100) + sz.data_chunk(b"") + filler(71, 1500, 100) + sz.data_chunk(b"", b"\x00") + filler(72, 1500, 100) + sz.data_chunk(b"")
    c.add("empty data chunks", s)
    # plain chunks whose payload is itself a complete .sz stream
    s, plain = ID, b""
    for k in range(5):
        inner = sz.write_sz_oracle(mix(2500, 80 + k), 200)
        s += sz.data_chunk(inner) + filler(90 + k, 600, 100)
    c.add("payloads that are .sz streams", s)
    # a payload full of hand-made 0x00 / 0x01 headers that chain to one another
    fake = b""
    for k in range(40):
        body = datagen.random_bytes(20 + 3 * k, seed=100 + k)
        fake += sz.chunk(0x01, bytes(4) + body) if k % 2 else sz.chunk(0x00, bytes(4) + rc.varint(len(body)) + rc.literal(body))
    s = ID + filler(120, 700, 100) + sz.data_chunk(fake) + filler(121, 700, 100) + sz.data_chunk(fake[7:] + fake[:900]) + filler(122, 3000, 100)
    c.add("a payload full of headers", s)
    c.add("small behind", sz.intact_streams()["two_files"][0])
    return [c]


# ---- damage ----
@functools.lru_cache(maxsize=None)
def damage_cases():
    """every damaged stream of sz_cases as the first bytes of a large item, in a middle segment, and as its last bytes"""
    seg = 1024
    out = []
    damaged = sz.damaged_streams()
    front, tail = ID + filler(130, 5000, 300), filler(131, 4000, 300)
    for where in ("first", "middle", "last"):
        c = Case("damage_" + where, seg)
        for name, d in damaged.items():
            s = {"first": d + tail, "middle": front + d + tail, "last": front + d}[where]
            if len(s) > seg:
                c.add(name, s, slack=(0, 9)[len(c.items) % 2])
        c.add("small intact behind", sz.intact_streams()["zero_length_chunks"][0])
        out.append(c)
    c = Case("damage_order", 512)
    third = ID + filler(140, 4000, 200)
    rest = filler(141, 8000, 200)
    c.add("small damaged in front", damaged["truncated_by_1"])
    c.add("0x02 at one third, then a truncated end", third + sz.chunk(0x02, b"what") + rest[:-1])
    c.add("a chunk with L 3 at one third, then 0x02", third + sz.chunk(0x01, b"abc") + rest[:3000] + sz.chunk(0x02, b"what") + rest[3000:])
    c.add("a truncated end alone", third + rest[:-1])
    c.add("0x7f as the last chunk", third + rest + sz.chunk(0x7f, b""))
    # bad chunks behind several joins: the number is the one within the item
    p = mix(500, 142)
    undecodable = sz.data_chunk(p, rc.varint(500) + rc.literal(p[:400]) + rc.copy2(64, 5000) + rc.literal(p[:36]))
    wrong_crc = sz.data_chunk(p, crc=0x12345678)
    c.add("an undecodable chunk behind several joins", third + rest[:len(rest) // 2] + undecodable + rest[len(rest) // 2:])
    c.add("a CRC mismatch behind several joins", third + rest + wrong_crc)
    c.add("two bad chunks", third + wrong_crc + rest + undecodable + filler(143, 1000, 100))
    c.add("two bad chunks, the other order", third + undecodable + rest + wrong_crc, slack=4)
    out.append(c)
    return out


# ---- limits ----
@functools.lru_cache(maxsize=None)
def limit_cases():
    out = []
    a = sz.write_sz_oracle(mix(9000, 150), 300)          # 30 chunks
    b = sz.write_sz_oracle(mix(12000, 151), 400)         # 30 chunks
    small, small_plain = sz.intact_streams()["two_files"]
    c = Case("limit_max_chunks", 1024, max_chunks=45)
    c.add("small", small).add("large inside", a).add("large beyond max_chunks", b).add("small behind the cut", small)
    out.append(c)
    c = Case("limit_max_chunks_0", 1024, max_chunks=0)
    c.add("large", a).add("identifier alone", ID)
    out.append(c)
    c = Case("limit_max_segments", 1024, max_segments=segments(len(a), 1024) + segments(len(b), 1024) - 1)
    c.add("large inside", a).add("small", small).add("large beyond max_segments", b).add("large behind it", a, slack=1)
    out.append(c)
    c = Case("limit_max_segments_0", 1024, max_segments=0)
    c.add("large", a).add("small", small)
    out.append(c)
    c = Case("sizing", 1024)
    c.add("capacity 0", a, capacity=0).add("null dst", b, capacity=len(mix(12000, 151)), item_flags=2).add("one byte short", a, capacity=8999)
    c.add("null src", a, capacity=16, item_flags=1).add("src_len above the maximum", a, capacity=16, src_len=0x7ffff001)
    c.add("damaged, capacity 0", sz.damaged_streams()["reserved_unskippable_02"] + filler(152, 3000, 200), capacity=0)
    out.append(c)
    c = Case("no_verify", 512, flags=sz.NO_VERIFY)
    p = mix(500, 142)
    c.add("a wrong CRC word", ID + filler(153, 4000, 200) + sz.data_chunk(p, crc=1) + filler(154, 3000, 200))
    c.add("an undecodable chunk", ID + filler(153, 4000, 200) + sz.data_chunk(p, rc.varint(500) + rc.literal(p[:400]) + rc.copy2(64, 5000) + rc.literal(p[:36])))
    c.add("small with a wrong CRC", sz.damaged_streams()["crc_word_bit_chunk2"])
    out.append(c)
    return out


def all_cases():
    return geometry_cases() + content_cases() + damage_cases() + limit_cases()


def case_names():
    return ["geometry_1024", "geometry_256", "geometry_4096", "contents_512", "damage_first", "damage_middle", "damage_last", "damage_order",
            "limit_max_chunks", "limit_max_chunks_0", "limit_max_segments", "limit_max_segments_0", "sizing", "no_verify"]


def case(name):
    group = {"geometry": geometry_cases, "contents": content_cases, "damage": damage_cases}.get(name.split("_")[0], limit_cases)
    return next(c for c in group() if c.name == name)


def count_data_chunks(stream):
    """the data chunks of a stream whose chain parses"""
    at = n = 0
    while at < len(stream):
        n += stream[at] <= 1
        at += 4 + int.from_bytes(stream[at + 1:at + 4], "little")
    return n


def expected_items(case):
    """-> per item (status, out_len, plaintext / pieces / None, bad_chunk) as sz_cases.read_sz states them, with what the call
    settles in front of any walk (a null src, src_len above the maximum) and the max_chunks cut over the items in order; and
    d_result[0], the data chunks the batch needs."""
    out, first = [], 0
    for _, s, cap, fl, n in case.items:
        if fl & 1:
            e = (sz.INVALID, 0, None, sz.NONE)
        elif n > rc.RAW_MAX_LEN:
            e = (sz.TOO_LARGE, 0, None, sz.NONE)
        else:
            e = sz.read_sz(s[:n], 0 if fl & 2 else cap, not case.flags & sz.NO_VERIFY)
            if e[0] == sz.OK or e[3] != sz.NONE:                 # the chain parses and the output fits: its chunks are planned
                k = count_data_chunks(s[:n])
                if k and first + k > case.max_chunks:
                    e = (sz.TOO_LARGE, e[1], None, sz.NONE)
                first += k
        out.append(e)
    return out, first
