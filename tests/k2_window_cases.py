"""Blocks for the check that K2 writes nothing outside a block's output window (k2_decode_block, csrc/snappy_kernels.hpp):
every block is decoded ALONE into a buffer of exactly its output length -- behind and in front of inaccessible pages on
the wave emulator (tests/test_k2_window_emulated.py), between guard bytes on the GPU (tests/test_gpu_k2_window.py).
Test infrastructure only: plain Python + the oracle.

A job is (name, stream, at, out_len): the block whose u32 size word is at stream[at] is to be decoded into out_len
bytes.  expect() gives what the oracle makes of that block alone; K2 may reject what the oracle accepts, never the other
way round, and accepted bytes are equal."""
import numpy as np

import datagen
import oracle_lib as oracle
import reference_cases as rc

M32 = 0xffffffff
OUT_LENS = (1, 63, 64, 65, 65535)


def _varint(v):
    return datagen._varint(v)


def expect(stream, at, out_len):
    """-> (status, bytes or None) of the oracle for the one block at `at`, as a container of its own."""
    if at + 4 > len(stream):
        return 1, None
    csz = int.from_bytes(stream[at:at + 4], "little")
    if at + 4 + csz > len(stream):
        return 1, None
    one = _varint(out_len) + _varint(max(out_len, 1)) + stream[at:at + 4 + csz]
    try:
        st, out = oracle.decompress(one)
    except ValueError:
        return 1, None
    return (0, out) if st == 0 else (1, None)


# ---- blocks of intact and damaged element streams ----------------------------------------------------------------------

def _offsets(stream):
    total, bs, hdr = oracle.read_header(stream)
    offs, at = [], hdr
    for _ in range((total + bs - 1) // bs):
        offs.append(at)
        at += 4 + int.from_bytes(stream[at:at + 4], "little")
    assert at == len(stream)
    return total, bs, offs


INTACT_BLOCK_SIZES = (64, 700, 4097, 32768, 65535)


def intact_containers():
    """(name, stream, plaintext): element streams of flavours 0-3, a few blocks each, the last one partial."""
    out = []
    for flavour in range(4):
        for k, bs in enumerate(INTACT_BLOCK_SIZES):
            total = 3 * bs + 17 + k if bs <= 4097 else bs + 3000 + 501 * k
            stream, plain = datagen.element_stream(total, bs, 600 * flavour + k, flavour)
            out.append(("elem-f%d-bs%d" % (flavour, bs), stream, plain))
    return out


PLANNER_TRIP_CONTAINERS = 1031


def planner_trip_containers():
    """[(stream, offsets, total_len, block_size)]: more containers than one trip of check_plan_kernel (1,024) -- one-block
    containers of at most 64 bytes, every eleventh damaged (its block starts with a copy: nothing to copy from), and as
    container 1024, the first of the second trip, one of four blocks whose block 2 is damaged."""
    kinds = []
    for k in range(5):
        stream, _ = datagen.element_stream(40 + 5 * k, 64, 900 + k, k % 4)
        total, bs, offs = _offsets(stream)
        bad = bytearray(stream)
        bad[offs[0] + 4] = 0xFF
        kinds.append(((stream, offs, total, bs), (bytes(bad), offs, total, bs)))
    stream, _ = datagen.element_stream(3 * 64 + 20, 64, 910, 0)
    total, bs, offs = _offsets(stream)
    bad = bytearray(stream)
    bad[offs[2] + 4] = 0xFF
    out = [kinds[i % 5][i % 11 == 7] for i in range(PLANNER_TRIP_CONTAINERS)]
    out[1024] = (bytes(bad), offs, total, bs)
    assert len(offs) == 4
    return out


def intact_jobs():
    jobs = []
    for name, stream, _ in intact_containers():
        total, bs, offs = _offsets(stream)
        for b, at in enumerate(offs):
            jobs.append(("%s-b%d" % (name, b), stream, at, min(bs, total - b * bs)))
    return jobs


def damaged_jobs(count=300):
    """The recipe of the damaged-stream tests (reference_cases.damaged_element_streams), `count` streams; a job for every
    block that holds a damaged byte, at the offset the block has in the undamaged stream."""
    jobs = []
    r = np.random.default_rng(31337)
    for k in range(count):
        bs = int(r.choice([700, 4097, 32768]))
        stream, _ = datagen.element_stream(int(r.integers(2_000, 60_000)), bs, 40_000 + k, k % 4)
        total, _, offs = _offsets(stream)
        b = bytearray(stream)
        hit = set()
        for _ in range(int(r.integers(1, 4))):
            at = int(r.integers(offs[0] + 4, len(b)))
            b[at] = int(r.integers(0, 256))
            hit.add(max(i for i, o in enumerate(offs) if o <= at))
        for i in sorted(hit):
            jobs.append(("damaged%d-b%d" % (k, i), bytes(b), offs[i], min(bs, total - i * bs)))
    return jobs


# ---- hand-made blocks aimed at the bound check `op + total > out_len` and its neighbours ------------------------------------

def _payload(k, salt=0):
    return bytes((i * 7 + 3 + salt) & 0xff for i in range(k))


def _literal(payload, length_bytes=None):
    n = len(payload) - 1
    if length_bytes is None:
        length_bytes = 0 if n < 60 else (1 if n < 256 else 2)
    if length_bytes == 0:
        return bytes([n << 2]) + payload
    return bytes([(59 + length_bytes) << 2]) + n.to_bytes(length_bytes, "little") + payload


def _fill(k):
    """k output bytes as literals of at most 60: 61 compressed bytes each, so what follows meets every window alignment."""
    out, done = b"", 0
    while done < k:
        step = min(60, k - done)
        out += _literal(_payload(step, done))
        done += step
    return out


def _raw_literal4(field, payload):
    return bytes([63 << 2]) + (field & M32).to_bytes(4, "little") + payload


def _copy2(length, offset):
    return bytes([2 | ((length - 1) << 2)]) + offset.to_bytes(2, "little")


def hand_bodies(L):
    """(name, compressed body) for an output window of L bytes."""
    v = []
    # a literal with a 4-byte length field, at the start of the block, a few bytes in, and near the end of the window
    for op in sorted({0, min(5, L - 1), max(L - 70, 0)}):
        left = L - op
        for tagname, length in (("len=ffffffff", M32), ("len=fffffffe", M32 - 1), ("len=left", left), ("len=left+1", left + 1),
                                ("len=left+2^32-64", (left + (1 << 32) - 64) & M32)):
            for how, field in (("field=len-1", length - 1), ("field=len", length)):
                have = length if length <= L + 1 else 70
                v.append(("lit4 op=%d %s %s" % (op, tagname, how), _fill(op) + _raw_literal4(field, _payload(have))))
    # one 64-byte window of elements whose lengths sum past 2^32
    for op in (0, min(3, L - 1)):
        v.append(("window sums past 2^32 op=%d" % op, _fill(op) + _raw_literal4(0x3fffffff, b"") * 5 + _payload(8)))
        v.append(("window sums past 2^16 op=%d" % op, _fill(op) + (bytes([61 << 2]) + b"\xff\xff") * 6 + _payload(8)))
    # 22 copies of 64 bytes in one window: the most a window can produce
    v.append(("22 copies of 64", _fill(1) + _copy2(64, 1) * 22))
    # a copy that ends exactly at, and 1 byte past, the window (a 64-byte one where the window has room for it)
    n = min(64, L - 1)
    if n >= 1:
        v.append(("copy%d ends at out_len" % n, _fill(L - n) + _copy2(n, 1)))
    n = min(64, L)
    v.append(("copy%d ends 1 past out_len" % n, _fill(L - n + 1) + _copy2(n, 1)))
    v.append(("copy64 from op=1", _fill(1) + _copy2(64, 1)))
    # a literal whose payload spills out of its 64-byte window of compressed data (and, longer, beyond the prefetched 128)
    for k in sorted({min(L, 66), min(L, 200), min(L, 5000)}):
        for nb in (None, 4):
            v.append(("spill literal %d ends at out_len nb=%s" % (k, nb), _fill(L - k) + _literal(_payload(k), nb)))
            v.append(("spill literal %d ends 1 past out_len nb=%s" % (k + 1, nb), _fill(L - k) + _literal(_payload(k + 1), nb)))
    return v


def hand_jobs():
    jobs = []
    for L in OUT_LENS:
        for name, body in hand_bodies(L):
            # as a stream of its own, with bytes behind the block that a decoder running on would pick up
            stream = _varint(L) + _varint(L) + len(body).to_bytes(4, "little") + body
            at = len(stream) - 4 - len(body)
            jobs.append(("hand L=%d %s" % (L, name), stream + _payload(40, 9), at, L))
            jobs.append(("hand L=%d %s (block ends the stream)" % (L, name), stream, at, L))
    return jobs


def check_job(job, st, out):
    """-> problem text or None for K2's answer (st, out bytes) to one job."""
    name, stream, at, out_len = job
    want_st, want = expect(stream, at, out_len)
    if st not in (0, 1):
        return "%s: status %r" % (name, st)
    if st == 0 and want_st != 0:
        return "%s: K2 accepts what the oracle rejects" % name
    if st == 0 and out != want:
        return "%s: accepted bytes differ from the oracle's" % name
    return None


def must_accept(job):
    """Blocks that are valid by construction: intact element streams, and the hand-made ones whose last element ends
    exactly at out_len with a minimal or 4-byte length field.  K2 must accept them (with the oracle's bytes)."""
    name = job[0]
    if name.startswith("elem-"):
        return True
    return name.startswith("hand ") and ("ends at out_len" in name or "len=left field=len-1" in name)
