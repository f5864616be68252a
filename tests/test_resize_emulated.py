"""CPU tests of the container resize: the UNMODIFIED kernels of pim-compression_amd/csrc/snappy_resize.hpp (with the update's
sizes and merge kernels, K2's decoder and K1's LDS-table form) on the lockstep wave emulator.  The acceptance test is an
identity with no tolerance: resize(container, keep_len, segments) == oracle.compress(plaintext[:keep_len] + the segments' bytes),
byte for byte.  Every run has 64 guard bytes around the new stream and guard words around the offsets, and compares the old
stream with its copy afterwards."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import datagen
import oracle_lib as oracle
import ranges_cases as rc
import resize_cases as rz
from conftest import golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None
PAD = 64                       # guard bytes in front of and behind the new stream
GUARD64 = 0x5A5A5A5A5A5A5A5A
SEGMENT_DTYPE = np.dtype([("src", "<u8"), ("length", "<u8")])   # snappy_hip_segment


def emu_lib():
    """tests/emu/emu_resize.cpp in a library of its own (the emulator runtime + the resize kernels)."""
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_resize.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_resize.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_ranges.hpp",
                                             "snappy_update.hpp", "snappy_resize.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.emu_resize.restype = ctypes.c_int
        L.emu_resize.argtypes = [vp, u64, vp, u32, u32, u32, u32, u32, u32, u32, vp, u32, vp, vp, u64, vp, vp, vp, u32, ctypes.c_int]
        _LIB = L
    return _LIB


class Result:
    pass


def run(c, keep_len, segments, new_total=None, capacity=None, grid=3, form=3, stream=None, desc_shape=None):
    """segments: list of bytes or (data, length, null src).  new_total: the host's new_total_len when it is not to be keep_len +
    the lengths.  stream: the bytes to resize instead of the container's own (a damaged copy; same offsets).  desc_shape:
    (total_len, block_size, num_blocks) of the descriptor when it is to differ from the host's copies."""
    old = np.frombuffer(c.stream if stream is None else stream, dtype=np.uint8).copy()
    offs = np.ascontiguousarray(c.offsets, dtype=np.uint64) if c.num_blocks else np.zeros(1, dtype=np.uint64)
    nb, bs = c.num_blocks, c.block_size
    keep = []
    arr = np.zeros(max(len(segments), 1), dtype=SEGMENT_DTYPE)
    total = keep_len
    for i, s in enumerate(segments):
        data, length, null = (s, len(s), False) if isinstance(s, bytes) else s
        # sources at every alignment: behind i % 16 + 1 spare bytes
        buf = np.frombuffer(bytes(i % 16 + 1) + data, dtype=np.uint8).copy()
        keep.append(buf)
        arr[i] = (0 if null else buf.ctypes.data + i % 16 + 1, length)
        total += length
    if new_total is None:
        new_total = total
    new_nb = (new_total + bs - 1) // bs
    if capacity is None:
        capacity = 10 + new_nb * ((4 + 32 + bs + bs // 6 + 15) & ~15)
    out = np.full(capacity + 2 * PAD, rz.GUARD, dtype=np.uint8)
    new_offs = np.full(new_nb + 3, GUARD64, dtype=np.uint64)
    new_len = np.full(1, GUARD64, dtype=np.uint64)
    result = np.full(2, 0x77, dtype=np.uint32)
    status = np.full(max(len(segments), 1), 0x55, dtype=np.uint32)
    dt, dbs, dnb = desc_shape or (c.total, bs, nb)
    unchanged = emu_lib().emu_resize(old.ctypes.data, old.size, offs.ctypes.data, dt, dbs, dnb, c.total, bs, keep_len, new_total, arr.ctypes.data,
                                     len(segments), status.ctypes.data, out.ctypes.data + PAD, capacity, new_offs.ctypes.data + 8,
                                     new_len.ctypes.data, result.ctypes.data, grid, form)
    assert unchanged in (0, 1), "no address space for the scratch"
    r = Result()
    r.old_unchanged = bool(unchanged)
    r.status = [int(x) for x in status[:len(segments)]]
    r.result = [int(x) for x in result]
    r.new_len = int(new_len[0])
    r.out, r.capacity = out, capacity
    r.new_offs, r.new_nb = new_offs, new_nb
    r.stream = out[PAD:PAD + r.new_len].tobytes() if r.new_len <= capacity else None
    return r


def assert_untouched(r):
    """REJECTED: not one byte of the new stream or the new offsets is written, the length reads 0."""
    assert r.old_unchanged
    assert r.result[0] == rz.REJECTED, r.result
    assert r.new_len == 0
    assert (r.out == rz.GUARD).all()
    assert (r.new_offs == GUARD64).all()


def check_ok(c, keep_len, segments, want=None, **kw):
    """segments: list of bytes.  want: the stream it must give when that is not only the oracle's (a golden)."""
    r = run(c, keep_len, segments, **kw)
    stream, want_offs, compressed = rz.expected(c, keep_len, segments)
    assert want is None or want == stream
    assert r.old_unchanged
    assert r.status == [0] * len(segments), r.status
    assert r.result == [rz.OK, compressed], r.result
    assert r.new_len == len(stream)
    assert r.stream == stream, next(i for i in range(len(stream)) if r.stream[i] != stream[i])
    assert [int(x) for x in r.new_offs[1:r.new_nb + 2]] == want_offs
    # guard bytes around the new stream and around the offsets
    assert (r.out[:PAD] == rz.GUARD).all() and (r.out[PAD + r.new_len:] == rz.GUARD).all()
    assert int(r.new_offs[0]) == GUARD64 and int(r.new_offs[r.new_nb + 2]) == GUARD64
    return r


@pytest.mark.parametrize("name", ["alice", "coding", "terror2"])
def test_resize_golden_identity(name):
    """The reference's own streams: oracle.compress(first part) + the rest appended == the golden; the golden truncated == the
    oracle's stream of the prefix; truncate(append(golden, x)) == the golden."""
    plain, golden = golden_bytes(name + ".txt"), golden_bytes(name + ".snappy")
    g = rc.Container(plain, golden)
    bs, total = g.block_size, g.total
    cuts = [rz.boundary(total, bs, last=False) or total, total // 3, 0]         # a block boundary, the middle of a block, nothing kept
    for cut in cuts:
        first = rc.Container(plain[:cut], block_size=bs)
        r = check_ok(first, cut, [plain[cut:]], want=golden)
        assert r.stream == golden
        r = check_ok(g, cut, [])
        assert r.stream == oracle.compress(plain[:cut], bs)
    x = rz.tail_bytes(plain, total, 777, "random", seed=len(name))
    grown = check_ok(g, total, [x]).stream
    r = check_ok(rc.Container(plain + x, grown), total, [], want=golden)
    assert r.stream == golden


def _vs_oracle(c, keeps, tails_of, seed, **kw):
    i = 0
    for keep_len in keeps:
        for n in tails_of(keep_len):
            kind = rz.KINDS[i % 3]
            i += 1
            tail = rz.tail_bytes(c.plain, keep_len, n, kind, seed + i)
            r = check_ok(c, keep_len, [tail] if n else [], **kw)
            if kind == "same" and n == c.total - keep_len:
                assert r.stream == c.stream


@pytest.mark.parametrize("bs,n", [(1, 200), (7, 1500), (64, 5000), (4096, 30000), (32768, 70000), (65535, 136000)])
def test_resize_block_sizes_vs_oracle(bs, n):
    """Every keep_len of resize_cases.keep_lens with every tail of resize_cases.tail_lens, the three kinds of bytes in turn, on a
    container whose length is no multiple of the block size and on one whose length is.  (Blocks of 32 KiB and more: a subset
    that still cuts in front of, on and behind a boundary -- the emulator compresses some 30 KB/s.)"""
    text = golden_bytes("plrabn12.txt")
    data = datagen.text_random_interleave(text, n, seed=bs)
    c = rc.Container(data, block_size=bs)
    assert bs == 1 or c.total % bs
    even = rc.Container(data[:n // bs * bs - (bs if bs >= 4096 else 0)], block_size=bs)
    assert even.total % bs == 0 and even.num_blocks >= 1
    if bs <= 4096:
        _vs_oracle(c, rz.keep_lens(c.total, bs), lambda k: rz.tail_lens(k, bs), seed=bs, form=2 if bs == 4096 else 3)
        _vs_oracle(even, rz.keep_lens(even.total, bs), lambda k: rz.tail_lens(k, bs), seed=bs + 1)
    else:
        b = rz.boundary(c.total, bs)
        fill = lambda k: bs - k % bs
        _vs_oracle(c, [b - 1], lambda k: [0, fill(k) + 1], seed=bs)             # the cut block decoded; filled and one byte more
        _vs_oracle(c, [b, b + 1], lambda k: [0, 1], seed=bs + 1)                # on the boundary nothing is decoded
        _vs_oracle(c, [c.total - 1, c.total], lambda k: [0, 1], seed=bs + 2)
        _vs_oracle(c, [c.total], lambda k: [fill(k)], seed=bs + 3)              # the short last block filled exactly
        _vs_oracle(c, [0, 1], lambda k: [0, 1], seed=bs + 4)
        _vs_oracle(even, [even.total], lambda k: [0, 1, fill(k) + 1], seed=bs + 5)


def test_resize_header_thresholds():
    """varint(total_len) grows by a byte at 128 and at 16384: every kept block's new offset is its old one plus or minus 1."""
    bs = 64
    text = golden_bytes("plrabn12.txt")
    for small in (127, 16383):
        a = rc.Container(text[:small], block_size=bs)
        b = rc.Container(text[:small + 1], block_size=bs)
        assert b.header_len == a.header_len + 1
        kept = small // bs
        up = check_ok(a, small, [text[small:small + 1]])
        assert up.stream == b.stream
        assert [int(x) for x in up.new_offs[1:1 + kept]] == [int(x) + 1 for x in a.offsets[:kept]]
        down = check_ok(b, small, [])
        assert down.stream == a.stream
        assert [int(x) for x in down.new_offs[1:1 + kept]] == [int(x) - 1 for x in b.offsets[:kept]]


@pytest.mark.parametrize("small,large", [(200, 300), (500, 600), (16000, 17000)])
def test_resize_table_size_thresholds(small, large):
    """K1 sizes its hash table by the block's length (256 entries up to 256 bytes, 512 up to 512, ... 16384 from 16384 up): a
    single short block grown and shrunk across a step comes out as the oracle compresses a block of the new length."""
    text = golden_bytes("plrabn12.txt")
    a = rc.Container(text[:small], block_size=32768)
    b = rc.Container(text[:large], block_size=32768)
    assert check_ok(a, small, [text[small:large]]).stream == b.stream
    assert check_ok(b, small, []).stream == a.stream


def test_resize_segments():
    bs = 64
    text = golden_bytes("terror2.txt")
    c = rc.Container(text[:1000], block_size=bs)
    # one tail as 1-byte segments across two block boundaries, with segments of length 0 between them (one with a null src)
    tail = rz.tail_bytes(c.plain, 990, 150, "random", seed=1)
    pieces = []
    for i, byte in enumerate(tail):
        pieces.append(bytes([byte]))
        if i % 7 == 3:
            pieces.append(b"")
    null_at = pieces.index(b"", 9)
    r = run(c, 990, [p if k != null_at else (b"", 0, True) for k, p in enumerate(pieces)])
    assert r.status == [0] * len(pieces) and r.result[0] == rz.OK
    assert r.stream == rz.expected(c, 990, pieces)[0] == check_ok(c, 990, [tail]).stream
    # 300 segments of mixed lengths, sources at every alignment, the three kinds of bytes
    for kind in rz.KINDS:
        tail = rz.tail_bytes(c.plain, 555, sum(rz.mixed_lengths(300, seed=2)), kind, seed=2)
        pieces = rz.split(tail, rz.mixed_lengths(300, seed=2))
        assert len(pieces) >= 300
        check_ok(c, 555, pieces)
    # a segment that spans three blocks between two short ones
    tail = rz.tail_bytes(c.plain, 1000, 10 + 3 * bs + 9, "zeros")
    check_ok(c, 1000, [tail[:10], tail[10:10 + 3 * bs], tail[10 + 3 * bs:]])
    check_ok(c, 30, rz.split(rz.tail_bytes(c.plain, 30, 400, "random", seed=4), [3 * bs + 1, 0, 17]), form=2)


def test_resize_grid_size_does_not_change_the_bytes():
    c = rc.Container(golden_bytes("terror2.txt")[:9000], block_size=1024)
    pieces = rz.split(rz.tail_bytes(c.plain, 4500, 6000, "random", seed=3), [700, 1, 2048])
    a = check_ok(c, 4500, pieces, grid=1)
    b = check_ok(c, 4500, pieces, grid=40)             # more wavefronts than new blocks
    assert a.out.tobytes() == b.out.tobytes()


def test_resize_empty_ends():
    e = rc.Container(b"", block_size=4096)
    text = golden_bytes("alice.txt")
    assert check_ok(e, 0, [text[:100], text[100:]]).stream == oracle.compress(text, 4096)
    assert check_ok(e, 0, []).stream == oracle.compress(b"", 4096)
    c = rc.Container(golden_bytes("coding.txt"), block_size=4096)
    assert check_ok(c, 0, []).stream == oracle.compress(b"", 4096)
    assert check_ok(c, 0, [b""]).stream == oracle.compress(b"", 4096)
    # keep_len == total_len without a tail: the stream again, the chain checked
    assert check_ok(c, c.total, []).stream == c.stream
    even = rc.Container(golden_bytes("coding.txt")[:8192], block_size=4096)
    assert check_ok(even, even.total, []).result == [rz.OK, 0]
    at = int(even.offsets[1])
    broken = bytearray(even.stream)
    broken[at:at + 4] = (int.from_bytes(broken[at:at + 4], "little") + 1).to_bytes(4, "little")
    assert run(even, even.total, [], stream=bytes(broken)).result[0] == rz.INVALID


def test_resize_rejected_causes_alone_and_mixed():
    """On a container whose last block is short and on one whose length is a multiple of the block size."""
    text = golden_bytes("terror2.txt")
    for c in (rc.Container(text[:20000], block_size=4096), rc.Container(text[:16384], block_size=4096)):
        for keep_len, segments, new_total, want, capacity in rz.rejected_cases(c):
            r = run(c, keep_len, segments, new_total=new_total, capacity=capacity)
            assert r.status == want, (keep_len, r.status)
            assert_untouched(r)
            assert r.result[1] == 0
    c = rc.Container(text[:20000], block_size=4096)
    keep, good = 10000, [b"abc", b"defgh"]
    assert run(c, keep, [(b"", 0, True), b"xyz"]).result[0] == rz.OK             # a null src with no bytes is allowed
    # capacity one byte short, then exact
    tail = [rz.tail_bytes(c.plain, keep, 9000, "random", seed=1)]
    need = len(rz.expected(c, keep, tail)[0])
    r = run(c, keep, tail, capacity=need - 1)
    assert r.status == [0] and r.result == [rz.REJECTED, rz.expected(c, keep, tail)[2]]
    assert_untouched(r)
    check_ok(c, keep, tail, capacity=need)
    # a descriptor of another shape
    for shape in [(c.total - 1, 4096, c.num_blocks), (c.total, 2048, c.num_blocks), (c.total, 4096, c.num_blocks - 1)]:
        assert_untouched(run(c, keep, good, desc_shape=shape))
    r = run(c, c.total + 1, good, desc_shape=(c.total, 2048, c.num_blocks), new_total=5)
    assert_untouched(r)


def test_resize_invalid_container():
    c = rc.Container(golden_bytes("terror2.txt")[:40000], block_size=4096)
    bs = 4096
    at = int(c.offsets[3])
    size = int.from_bytes(c.stream[at:at + 4], "little")
    broken = bytearray(c.stream)
    broken[at:at + 4] = (size - 1).to_bytes(4, "little")          # block 3: the link does not hold, and it ends inside its last element
    broken = bytes(broken)
    inside = bytearray(c.stream)
    inside[at + 4] = 0xFF                                          # block 3's first element a copy: nothing to refer to
    inside = bytes(inside)
    tail = [b"the tail"]
    # a broken link in a kept block
    r = run(c, 5 * bs + 7, tail, stream=broken)
    assert r.old_unchanged and r.status == [0] and r.result == [rz.INVALID, rz.expected(c, 5 * bs + 7, tail)[2]] and r.new_len == 0
    assert run(c, 4 * bs, [], stream=broken).result[0] == rz.INVALID
    # the cut block does not decode: both damages
    for stream in (broken, inside):
        r = run(c, 3 * bs + 5, tail, stream=stream)
        assert r.old_unchanged and r.status == [0] and r.result == [rz.INVALID, 1] and r.new_len == 0
    # the same damage in a block wholly behind keep_len, and in the cut block's place with keep_len on the boundary in front of
    # it (nothing is decoded): OK, the oracle's bytes
    for stream in (broken, inside):
        for keep_len in (2 * bs + 100, 3 * bs - 1, 3 * bs, 0):
            check_ok(c, keep_len, tail, stream=stream)
            check_ok(c, keep_len, [], stream=stream)
    # damage inside a kept block's payload with an intact link travels along unchanged
    r = run(c, 6 * bs + 1, tail, stream=inside)
    assert r.result[0] == rz.OK
    assert r.stream[int(r.new_offs[4]):int(r.new_offs[5])] == inside[at:int(c.offsets[4])]
    want = rz.expected(c, 6 * bs + 1, tail)[0]
    assert r.new_len == len(want) and r.stream[int(r.new_offs[5]):] == want[int(r.new_offs[5]):]
