"""CPU tests of the container update: the UNMODIFIED kernels of pim-compression_amd/csrc/snappy_update.hpp (with K2's decoder
and K1's LDS-table form from snappy_kernels.hpp) on the lockstep wave emulator.  The acceptance test is an identity with no
tolerance: update(container, writes) == oracle.compress(plaintext with the writes applied), byte for byte."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import datagen
import oracle_lib as oracle
import ranges_cases as rc
import update_cases as uc
from conftest import golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None
PAD = 64                       # guard bytes in front of and behind the new stream
GUARD64 = 0x5A5A5A5A5A5A5A5A


def emu_lib():
    """tests/emu/emu_update.cpp in a library of its own (the emulator runtime + the update kernels)."""
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_update.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_update.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_ranges.hpp", "snappy_update.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.emu_update_ranges.restype = ctypes.c_int
        L.emu_update_ranges.argtypes = [vp, u64, vp, u32, u32, u32, u32, u32, vp, u32, vp, vp, u64, vp, vp, vp, u32, u32, ctypes.c_int]
        _LIB = L
    return _LIB


class Result:
    pass


def run(c, writes, max_dirty=None, capacity=None, grid=3, form=3, stream=None, desc_shape=None):
    """writes: list of (offset, data) or (offset, data, length, null src).  stream: the bytes to update instead of the
    container's own (a damaged copy; same offsets).  desc_shape: (total_len, block_size, num_blocks) of the descriptor when it
    is to differ from the host's copies."""
    old = np.frombuffer(c.stream if stream is None else stream, dtype=np.uint8).copy()
    offs = np.ascontiguousarray(c.offsets, dtype=np.uint64) if c.num_blocks else np.zeros(1, dtype=np.uint64)
    nb = c.num_blocks
    keep = []
    arr = np.zeros(max(len(writes), 1), dtype=[("offset", "<u8"), ("length", "<u8"), ("src", "<u8"), ("pad", "<u8")])
    for i, w in enumerate(writes):
        off, data = w[0], w[1]
        length = w[2] if len(w) > 2 else len(data)
        null = w[3] if len(w) > 3 else False
        # sources at every alignment: behind i % 16 + 1 spare bytes
        buf = np.frombuffer(bytes(i % 16 + 1) + data, dtype=np.uint8).copy()
        keep.append(buf)
        arr[i] = (off, length, 0 if null else buf.ctypes.data + i % 16 + 1, 0)
    if max_dirty is None:
        max_dirty = max(nb, 1)
    if capacity is None:
        capacity = 10 + nb * ((4 + 32 + c.block_size + c.block_size // 6 + 15) & ~15)
    out = np.full(capacity + 2 * PAD, uc.GUARD, dtype=np.uint8)
    new_offs = np.full(nb + 3, GUARD64, dtype=np.uint64)
    new_len = np.full(1, GUARD64, dtype=np.uint64)
    result = np.full(2, 0x77, dtype=np.uint32)
    status = np.full(max(len(writes), 1), 0x55, dtype=np.uint32)
    dt, dbs, dnb = desc_shape or (c.total, c.block_size, nb)
    unchanged = emu_lib().emu_update_ranges(old.ctypes.data, old.size, offs.ctypes.data, dt, dbs, dnb, c.total, c.block_size, arr.ctypes.data,
                                            len(writes), status.ctypes.data, out.ctypes.data + PAD, capacity, new_offs.ctypes.data + 8,
                                            new_len.ctypes.data, result.ctypes.data, max_dirty, grid, form)
    r = Result()
    r.old_unchanged = bool(unchanged)
    r.status = [int(x) for x in status[:len(writes)]]
    r.result = [int(x) for x in result]
    r.new_len = int(new_len[0])
    r.out, r.capacity = out, capacity
    r.new_offs = new_offs
    return r


def assert_untouched(r):
    """REJECTED: not one byte of the new stream or the new offsets is written, the length reads 0."""
    assert r.old_unchanged
    assert r.result[0] == uc.REJECTED
    assert r.new_len == 0
    assert (r.out == uc.GUARD).all()
    assert (r.new_offs == GUARD64).all()


def check_ok(c, writes, **kw):
    """writes: list of (offset, data)."""
    r = run(c, writes, **kw)
    want, want_offs, dirty = uc.expected(c, writes)
    assert r.old_unchanged
    assert r.status == [0] * len(writes), r.status
    assert r.result == [uc.OK, dirty], r.result
    assert r.new_len == len(want)
    got = r.out[PAD:PAD + r.new_len].tobytes()
    assert got == want, next(i for i in range(len(want)) if got[i] != want[i])
    assert [int(x) for x in r.new_offs[1:c.num_blocks + 2]] == want_offs
    # guard bytes around the new stream and around the offsets
    assert (r.out[:PAD] == uc.GUARD).all() and (r.out[PAD + r.new_len:] == uc.GUARD).all()
    assert int(r.new_offs[0]) == GUARD64 and int(r.new_offs[c.num_blocks + 2]) == GUARD64
    return r


def with_data(c, ranges, kind, seed=0):
    return [(o, uc.new_bytes(c.plain, o, n, kind, seed)) for o, n in ranges]


@pytest.mark.parametrize("name", ["alice", "coding", "terror2"])
def test_update_goldens(name):
    """The reference's own streams: each write alone and the sets, in the three kinds of bytes.  (terror2, four blocks of
    32 KiB: the kinds take turns -- zeros and random bytes for the writes alone, all three over the sets -- because the emulator
    compresses some 30 KB/s.)"""
    c = rc.Container(golden_bytes(name + ".txt"), golden_bytes(name + ".snappy"))
    small = c.num_blocks == 1
    sets = uc.write_sets(c.total, c.block_size, seed=len(name), random_count=4 if small else 1)
    for i, ws in enumerate(sets):
        if small:
            kinds = uc.KINDS if len(ws) > 1 else (uc.KINDS[i % 3],)
        else:
            kinds = (uc.KINDS[i % 3],) if len(ws) > 1 else (uc.KINDS[1 + i % 2],)   # ("same" costs the emulator twice as much)
        for kind in kinds:
            r = check_ok(c, with_data(c, ws, kind, seed=i))
            if kind == "same":
                assert r.out[PAD:PAD + r.new_len].tobytes() == c.stream


@pytest.mark.parametrize("bs,n", [(1, 200), (7, 1500), (64, 5000), (4096, 30000), (32768, 70000), (65535, 136000)])
@pytest.mark.parametrize("kind", uc.KINDS)
def test_update_block_sizes_vs_oracle(bs, n, kind):
    text = golden_bytes("plrabn12.txt")
    c = rc.Container(datagen.text_random_interleave(text, n, seed=bs), block_size=bs)
    nb = c.num_blocks
    last = (nb - 1) * bs
    # one byte on both sides of block boundaries, and a write ending in the short last block
    ranges = uc.disjoint([(b * bs - 1, 1) for b in (1, nb // 2, nb - 1) if 0 < b < nb] + [(b * bs, 1) for b in (1, nb - 1) if 0 < b < nb] +
                         [(max(last - 3, 0), c.total - max(last - 3, 0))])
    assert bs == 1 or c.total - last < bs
    r = check_ok(c, with_data(c, ranges, kind, seed=bs))
    if kind == "same":
        assert r.out[PAD:PAD + r.new_len].tobytes() == c.stream
    # the whole container (large blocks: one kind per block size, the emulator compresses some 30 KB/s)
    if bs <= 4096 or kind == uc.KINDS[bs % 3]:
        check_ok(c, with_data(c, [(0, c.total)], kind, seed=bs + 1))
    if bs <= 4096:
        check_ok(c, with_data(c, uc.write_sets(c.total, bs, seed=bs, random_count=4)[-3], kind, seed=bs + 3), form=2 if bs == 4096 else 3)


def test_update_grid_size_does_not_change_the_bytes():
    c = rc.Container(golden_bytes("terror2.txt")[:60000], block_size=4096)
    ws = with_data(c, uc.disjoint([(100, 5000), (9000, 1), (20000, 12000), (50000, 9000)]), "random", seed=3)
    a = check_ok(c, ws, grid=1)
    b = check_ok(c, ws, grid=40)                       # more wavefronts than dirty blocks
    assert a.out.tobytes() == b.out.tobytes()


def test_update_writes_that_cover_a_block_together():
    """Adjacent writes that together cover blocks completely (no write does alone)."""
    c = rc.Container(golden_bytes("terror2.txt")[:30000], block_size=4096)
    cuts = [4000, 4100, 6000, 8192, 9000, 12288, 12289]
    check_ok(c, with_data(c, [(a, b - a) for a, b in zip(cuts, cuts[1:])], "random", seed=8))


def test_update_no_writes_and_empty_writes_copy_the_stream():
    c = rc.Container(golden_bytes("alice.txt"), golden_bytes("alice.snappy"))
    r = check_ok(c, [])
    assert r.out[PAD:PAD + r.new_len].tobytes() == c.stream
    r = check_ok(c, [(0, b""), (5, b""), (c.total // 2, b""), (c.total, b""), (c.total, b"")])
    assert r.out[PAD:PAD + r.new_len].tobytes() == c.stream
    check_ok(c, [(5, b""), (5, b"xyz"), (8, b""), (c.total, b"")], max_dirty=1)


def test_update_empty_container_gives_the_header():
    c = rc.Container(b"", block_size=32768)
    r = check_ok(c, [])
    assert r.out[PAD:PAD + r.new_len].tobytes() == oracle.compress(b"", 32768)
    check_ok(c, [(0, b"")])


def test_update_rejected_causes_alone_and_mixed():
    c = rc.Container(golden_bytes("terror2.txt")[:40000], block_size=4096)
    big = (1 << 64) - 1
    good = [(10, b"abc"), (5000, b"defgh")]
    cases = [
        ([(c.total - 2, b"xyz")], [uc.OUT_OF_BOUNDS]),                                  # one byte beyond the end
        ([(c.total + 1, b"")], [uc.OUT_OF_BOUNDS]),
        ([(big - 1, b"xy", 5, False)], [uc.OUT_OF_BOUNDS]),                              # offset + length overflows
        ([(7, b"", big, False)], [uc.OUT_OF_BOUNDS]),
        ([(7, b"", 3, True)], [uc.OUT_OF_BOUNDS]),                                       # null src
        ([(100, b"abc"), (50, b"de")], [0, uc.UNORDERED]),
        ([(100, b"abcd"), (103, b"de")], [0, uc.UNORDERED]),                             # overlapping by one byte
        (good + [(c.total - 2, b"xyz")], [0, 0, uc.OUT_OF_BOUNDS]),
        ([good[0], (4, b"z"), good[1]], [0, uc.UNORDERED, 0]),
        ([good[0], (20, b"", 3, True), (21, b"q"), good[1]], [0, uc.OUT_OF_BOUNDS, uc.UNORDERED, 0]),
        ([(big - 1, b"xy", 5, False), (9, b"a")], [uc.OUT_OF_BOUNDS, uc.UNORDERED]),     # behind an overflowing write: its end is "infinite"
    ]
    for writes, want in cases:
        r = run(c, writes)
        assert r.status == want, (writes, r.status)
        assert_untouched(r)
    assert run(c, [(7, b"", 0, True)]).result[0] == uc.OK                                # null src with no bytes is allowed


def test_update_rejected_for_one_dirty_block_too_many():
    c = rc.Container(golden_bytes("terror2.txt")[:40000], block_size=4096)
    writes = [(4095, b"ab"), (20000, b"c")]                                              # blocks 0, 1 and 4
    r = run(c, writes, max_dirty=2)
    assert r.status == [0, 0] and r.result == [uc.REJECTED, 3]
    assert_untouched(r)
    check_ok(c, writes, max_dirty=3)


def test_update_rejected_for_capacity_one_byte_short():
    c = rc.Container(golden_bytes("terror2.txt")[:40000], block_size=4096)
    writes = with_data(c, [(100, 9000)], "random", seed=1)
    need = len(uc.expected(c, writes)[0])
    r = run(c, writes, capacity=need - 1)
    assert r.status == [0] and r.result[0] == uc.REJECTED
    assert_untouched(r)
    check_ok(c, writes, capacity=need)


def test_update_descriptor_of_another_shape_is_rejected():
    c = rc.Container(golden_bytes("terror2.txt")[:40000], block_size=4096)
    for shape in [(c.total - 1, 4096, c.num_blocks), (c.total, 2048, c.num_blocks), (c.total, 4096, c.num_blocks - 1)]:
        assert_untouched(run(c, [(10, b"abc")], desc_shape=shape))


def test_update_invalid_container():
    c = rc.Container(golden_bytes("terror2.txt")[:40000], block_size=4096)
    bs = 4096
    at = int(c.offsets[3])
    size = int.from_bytes(c.stream[at:at + 4], "little")
    broken = bytearray(c.stream)
    broken[at:at + 4] = (size - 1).to_bytes(4, "little")          # block 3: the link does not hold, and it ends inside its last element
    broken = bytes(broken)
    # a broken link at a clean block
    r = run(c, [(10, b"abc")], stream=broken)
    assert r.old_unchanged and r.status == [0] and r.result[0] == uc.INVALID
    r = run(c, [], stream=broken)
    assert r.old_unchanged and r.result[0] == uc.INVALID
    # the damaged block dirty, partly overwritten: it has to decode, and does not
    r = run(c, [(3 * bs + 5, b"abc")], stream=broken)
    assert r.old_unchanged and r.status == [0] and r.result[0] == uc.INVALID
    # damage inside the payload with the link intact: a dirty block that does not decode
    inside = bytearray(c.stream)
    inside[at + 4] = 0xFF                                          # the block's first element a copy: nothing to refer to
    r = run(c, [(3 * bs + 5, b"abc")], stream=bytes(inside))
    assert r.old_unchanged and r.result[0] == uc.INVALID
    # ... overwritten completely it is not decoded at all: OK, with the oracle's bytes (by one write, and by two together)
    for stream in (broken, bytes(inside)):
        check_ok(c, with_data(c, [(3 * bs, bs)], "random", seed=5), stream=stream)
        check_ok(c, with_data(c, [(3 * bs - 7, 100), (3 * bs + 93, bs)], "zeros"), stream=stream)
    # ... and clean with the link intact it travels along as it is
    r = run(c, [(10, b"abc")], stream=bytes(inside))
    assert r.result[0] == uc.OK
    got = r.out[PAD:PAD + r.new_len].tobytes()
    assert got[int(r.new_offs[4]):int(r.new_offs[5])] == bytes(inside)[at:int(c.offsets[4])]
