"""Seeded cases for byte ranges of .sz streams (snappy_hip_sz_index_batch / snappy_hip_sz_decompress_ranges) and a model of
both calls in plain Python, over the streams and the reader of tests/sz_cases.py.  The model walks the chain as sz_cases.read_sz
does and judges ONLY the chunks a range touches: first = the largest k with dst_off[k] <= offset, last = the largest k with
dst_off[k] <= offset + length - 1, every data chunk between them included.  tests/test_sz_ranges_model.py holds it to read_sz."""
import collections
import random

import datagen
import raw_cases as rc
import sz_cases as sz

OK, INVALID, OUT_OF_BOUNDS, TOO_LARGE, CRC_MISMATCH, UNSUPPORTED = sz.OK, sz.INVALID, 2, sz.TOO_LARGE, sz.CRC_MISMATCH, sz.UNSUPPORTED
NONE = sz.NONE
U64 = 1 << 64

Chunk = collections.namedtuple("Chunk", "kind word body n src_off dst_off L hdr")


# ---- the model ----
def chain(s):
    """-> (status, [Chunk], total): read_sz's walk of the chain, with every data chunk's place; (status, [], 0) unless OK"""
    if len(s) > rc.RAW_MAX_LEN:
        return TOO_LARGE, [], 0
    at, identified, chunks, total = 0, False, [], 0
    while at < len(s):
        if at + 4 > len(s):
            return INVALID, [], 0
        kind, L = s[at], int.from_bytes(s[at + 1:at + 4], "little")
        if at + 4 + L > len(s):
            return INVALID, [], 0
        body = s[at + 4:at + 4 + L]
        if kind == 0xff:
            if body != b"sNaPpY":
                return INVALID, [], 0
            identified = True
        elif not identified:
            return INVALID, [], 0
        elif kind <= 1:
            if L < 4:
                return INVALID, [], 0
            n, hdr = L - 4, 0
            if kind == 0:
                h = rc.header_parses(body[4:])
                if h is None:
                    return INVALID, [], 0
                n, hdr = h
            if n > sz.MAX_CHUNK:
                return INVALID, [], 0
            chunks.append(Chunk(kind, int.from_bytes(body[:4], "little"), body[4:], n, at, total, L, hdr))
            total += n
        elif kind < 0x80:
            return UNSUPPORTED, [], 0
        at += 4 + L
    if not identified:
        return INVALID, [], 0
    if total > rc.RAW_MAX_LEN:
        return TOO_LARGE, [], 0
    return OK, chunks, total


def chunk_verdict(c, verify=True):
    """-> (status, plaintext or None) of one data chunk on its own"""
    st, piece = OK, c.body
    if c.kind == 0:
        st, _, piece = rc.expect(c.body, None)
    if st == OK and verify and sz.mask(sz.crc32c(piece)) != c.word:
        st = CRC_MISMATCH
    return st, (piece if st == OK else None)


def record(c, item=0):
    """the snappy_hip_sz_chunk of a chunk: (src_off, dst_off, info, ulen, item)"""
    return (c.src_off, c.dst_off, c.L | (c.hdr << 24) | ((1 << 28) if c.kind == 0 else 0), c.n, item)


def index_model(s):
    """-> (status, records, total_len) of one item of snappy_hip_sz_index_batch with room for all its chunks"""
    st, chunks, total = chain(s)
    return st, [record(c) for c in chunks], total


def touched(chunks, offset, length):
    """(first, last) of a range inside the plaintext, length > 0"""
    first = max(k for k, c in enumerate(chunks) if c.dst_off <= offset)
    last = max(k for k, c in enumerate(chunks) if c.dst_off <= offset + length - 1)
    return first, last


_VERDICTS = {}


def range_model(s, offset, length, verify=True):
    """-> (status, bad_chunk, bytes or None) of the range [offset, offset + length) of the stream s"""
    key = (id(s), verify)
    if key not in _VERDICTS:
        st, chunks, total = chain(s)
        _VERDICTS[key] = (s, chunks, total, [chunk_verdict(c, verify) for c in chunks])
    _, chunks, total, verdicts = _VERDICTS[key]
    if offset + length >= U64 or offset + length > total:
        return OUT_OF_BOUNDS, NONE, None
    if length == 0:
        return OK, NONE, b""
    first, last = touched(chunks, offset, length)
    out = bytearray()
    for k in range(first, last + 1):
        st, piece = verdicts[k]
        if st != OK:
            return st, k, None
        out += piece
    lo = offset - chunks[first].dst_off
    return OK, NONE, bytes(out[lo:lo + length])


# ---- the streams ----
def write_mixed(plain, seed, lo=64, hi=4096):
    """chunks of seeded lengths lo..hi, compressed by Google's Snappy where that is shorter, else of type 0x01"""
    import pyarrow as pa
    codec = pa.Codec("snappy")
    rng = random.Random(seed)
    out, at = bytearray(sz.IDENTIFIER), 0
    while at < len(plain):
        piece = plain[at:at + rng.randint(lo, hi)]
        raw = codec.compress(piece, asbytes=True)
        out += sz.data_chunk(piece, raw if len(raw) < len(piece) else None)
        at += len(piece)
    return bytes(out)


_STREAMS = None


def streams():
    """name -> (stream, plaintext): the intact streams the ranges run over"""
    global _STREAMS
    if _STREAMS is None:
        v = {}
        for name, n, seed in (("mixed_4k", 4096, 11), ("mixed_20k", 20000, 12), ("mixed_64k", 65536, 13)):
            plain = sz.text_random_mix(n, seed)
            v[name] = (write_mixed(plain, seed), plain)
        text = sz.text_random_mix(140000, 14)
        rnd = datagen.random_bytes(65536, seed=15)
        big = text[:65536] + rnd + text[65536:140000]
        import pyarrow as pa
        codec = pa.Codec("snappy")
        v["both_types_65536"] = (sz.IDENTIFIER + sz.data_chunk(big[:65536], codec.compress(big[:65536], asbytes=True)) + sz.data_chunk(rnd) +
                                 sz.data_chunk(big[131072:196608], codec.compress(big[131072:196608], asbytes=True)) + sz.data_chunk(big[196608:]), big)
        intact = sz.intact_streams()
        for name in ("padding_and_skippable", "two_files", "zero_length_chunks", "identifier_alone", "padded_varint"):
            v[name] = intact[name]
        _STREAMS = v
    return _STREAMS


def edge_ranges(s, seed=0, many=6):
    """[(offset, length)] inside one intact stream: the edges of its chunk table and `many` seeded ones"""
    st, chunks, total = chain(s)
    assert st == OK
    r = [(0, 0), (total // 2, 0), (total, 0)]
    if total == 0:
        return r
    real = [c for c in chunks if c.n]
    mid = real[len(real) // 2]
    r += [(mid.dst_off, 1), (mid.dst_off + mid.n - 1, 1), (mid.dst_off, mid.n), (total - 1, 1), (0, total), (0, 1)]
    if mid.n > 1:
        r += [(mid.dst_off, mid.n // 2), (mid.dst_off + mid.n // 2, mid.n - mid.n // 2)]           # chunk start to mid-chunk, and the reverse
    for span in (2, 3):
        if len(real) >= span + 1:
            a, b = real[1], real[span]
            r += [(a.dst_off + a.n // 2, b.dst_off + (b.n + 1) // 2 - a.dst_off - a.n // 2), (a.dst_off, b.dst_off + b.n - a.dst_off)]
    for k, c in enumerate(chunks):                                                                 # at and across empty chunks
        if c.n == 0 and c.dst_off < total:
            r += [(c.dst_off, min(5, total - c.dst_off))]
            if c.dst_off:
                r += [(c.dst_off - 1, min(3, total - c.dst_off + 1))]
    for k in range(len(chunks) - 1):                                                               # type 0x00 / 0x01 neighbours
        a, b = chunks[k], chunks[k + 1]
        if a.kind != b.kind and a.n and b.n:
            r += [(a.dst_off + a.n - 1, 2), (a.dst_off, a.n + b.n)]
            break
    rng = random.Random(seed)
    for _ in range(many):
        off = rng.randrange(total)
        r.append((off, rng.randint(1, total - off)))
    return r


def seeded_ranges(total, count, seed, longest):
    """`count` ranges of 1..longest bytes inside `total`, short ones as likely as long ones"""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.randint(1, min(rng.choice([64, 4096, 40000, longest]), total))
        out.append((rng.randrange(total - n + 1), n))
    return out


# A case: streams = [(label, bytes)], ranges = [(stream, offset, length, null_dst)], verify.  expected(case) -> per range
# (status, bad_chunk, bytes or None), per stream the index status.
Case = collections.namedtuple("Case", "name streams ranges verify")


def parsing_damage():
    """name -> stream: the damaged streams of sz_cases whose chain parses (the index call accepts them)"""
    return {k: s for k, s in sz.damaged_streams().items() if chain(s)[0] == OK}


def damage_ranges(s):
    """[(offset, length)] for one damaged stream whose chain parses: one range over every bad chunk (at least a byte of it, or
    what lies at its place), one over a good chunk beside it; for two bad chunks a range over both and one over the later alone"""
    _, chunks, total = chain(s)
    bad = [k for k, c in enumerate(chunks) if chunk_verdict(c)[0] != OK]
    good = [k for k, c in enumerate(chunks) if c.n and k not in bad]
    r = []
    for k in bad:
        c = chunks[k]
        if c.dst_off < total:
            r.append((c.dst_off, max(1, min(c.n, total - c.dst_off))))
    if len(bad) >= 2:
        a, b = chunks[bad[0]], chunks[bad[-1]]
        r.append((a.dst_off, b.dst_off + max(b.n, 1) - a.dst_off))
        r.append((b.dst_off + b.n // 2, max(1, b.n - b.n // 2)))
    for k in good[:2]:
        r.append((chunks[k].dst_off, chunks[k].n))
    if total:
        r.append((0, total))
    return r


_CASES = None


def all_cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    v = streams()
    for name, (s, plain) in v.items():
        rs = [(0, off, n, False) for off, n in edge_ranges(s, seed=len(out))]
        out.append(Case("edges_" + name, [(name, s)], rs, True))
    # several streams of one batch, one of them not indexed; overlapping ranges; the malformed requests
    bad_chain = sz.damaged_streams()["truncated_by_1"]
    names = ["mixed_20k", "zero_length_chunks", "two_files", "mixed_4k"]
    batch = [(n, v[n][0]) for n in names[:2]] + [("truncated_by_1", bad_chain)] + [(n, v[n][0]) for n in names[2:]]
    rs = []
    for i, (label, s) in enumerate(batch):
        if i == 2:
            rs += [(i, 0, 0, False), (i, 0, 1, False), (i, 5, 0, False)]
            continue
        total = chain(s)[2]
        rs += [(i, off, n, False) for off, n in edge_ranges(s, seed=100 + i, many=3)]
        rs += [(i, total // 4, total // 2, False), (i, total // 3, total // 2, False)]               # two ranges overlapping in the stream
        rs += [(i, total, 1, False), (i, 1, total, False), (i, U64 - 1, 2, False), (i, U64 - 8, 8, False), (i, 0, total, True), (i, 0, 0, True)]
    rs += [(len(batch), 0, 1, False), (len(batch), 0, 0, False), (0xffffffff, 0, 1, False)]
    out.append(Case("batch_and_malformed", batch, rs, True))
    out.append(Case("batch_no_verify", batch, rs, False))
    dmg = parsing_damage()
    for verify in (True, False):
        batch, rs = [], []
        for name, s in sorted(dmg.items()):
            rs += [(len(batch), off, n, False) for off, n in damage_ranges(s)]
            batch.append((name, s))
        out.append(Case("damage" if verify else "damage_no_verify", batch, rs, verify))
    _CASES = out
    return out


def case_names():
    return ["edges_" + n for n in ("mixed_4k", "mixed_20k", "mixed_64k", "both_types_65536", "padding_and_skippable", "two_files",
                                   "zero_length_chunks", "identifier_alone", "padded_varint")] + \
        ["batch_and_malformed", "batch_no_verify", "damage", "damage_no_verify"]


def case(name):
    return next(c for c in all_cases() if c.name == name)


def expected(c):
    """-> ([index status per stream], [(status, bad_chunk, bytes or None) per range])"""
    idx = [chain(s)[0] for _, s in c.streams]
    want = []
    for stream, off, n, null_dst in c.ranges:
        if stream >= len(c.streams):
            want.append((OUT_OF_BOUNDS, NONE, None))
            continue
        st, bad, data = range_model(c.streams[stream][1], off, n, c.verify)
        if null_dst and n and st != OUT_OF_BOUNDS:
            st, bad, data = OUT_OF_BOUNDS, NONE, None
        want.append((st, bad, data))
    return idx, want


# ---- a stale index: edits of one record after the index call ----
def stale_edits():
    """name -> f(record as a dict) editing it in place; each makes the record BLOCK_INVALID for the ranges that touch it"""
    def L_off_by_one(r):
        r["info"] += 1

    def src_off_past(r, src_len=None):
        r["src_off"] = 1 << 40

    def ulen_65537(r):
        r["ulen"] = 65537

    def type_flipped(r):
        r["info"] ^= 1 << 28

    return {"L_off_by_one": L_off_by_one, "src_off_past_src_len": src_off_past, "ulen_65537": ulen_65537, "type_bit_flipped": type_flipped}


def stale_case():
    """(label, stream, k, ranges): record k of the stream is edited; ranges = [(offset, length)] some touching k, some not"""
    s, plain = streams()["mixed_20k"]
    _, chunks, total = chain(s)
    k = len(chunks) // 2
    c = chunks[k]
    rs = [(c.dst_off, c.n), (c.dst_off + c.n - 1, 1), (chunks[k - 1].dst_off, c.dst_off + 1 - chunks[k - 1].dst_off), (0, total),
          (chunks[k - 1].dst_off, chunks[k - 1].n), (chunks[k + 1].dst_off, chunks[k + 1].n), (0, c.dst_off), (c.dst_off + c.n, total - c.dst_off - c.n)]
    return "mixed_20k", s, k, rs
