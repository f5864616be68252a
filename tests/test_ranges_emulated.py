"""CPU tests of the range decoder: the UNMODIFIED kernels of pim-compression_amd/csrc/snappy_ranges.hpp (range_pieces_kernel +
decompress_ranges_kernel, with K2's decoder from snappy_kernels.hpp) on the lockstep wave emulator, against oracle slices."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import datagen
import oracle_lib as oracle
import ranges_cases as rc
from conftest import golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def emu_lib():
    """tests/emu/emu_ranges.cpp in a library of its own (the emulator runtime + the range kernels)."""
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_ranges.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_ranges.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h"),
                os.path.join(csrc, "snappy_device_common.hpp"), os.path.join(csrc, "snappy_kernels.hpp"),
                os.path.join(csrc, "snappy_k1_stream.hpp"), os.path.join(csrc, "snappy_ranges.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        L.emu_decompress_ranges.restype = None
        L.emu_decompress_ranges.argtypes = [u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, u32, u32, u32]
        _LIB = L
    return _LIB


def run(containers, requests, dst_offsets=None, buf_len=None, slots=4, grid=3, max_block_size=None, streams=None):
    """requests: list of (container index, offset, length).  Returns (statuses, destination buffer, dst offsets).
    streams: the stream bytes to decode instead of the containers' own (a damaged copy; same block offsets)."""
    n = len(containers)
    keep = []
    stream_arrs = [np.frombuffer(s if streams is None else streams[i], dtype=np.uint8).copy() for i, s in
                   enumerate([c.stream for c in containers])]
    offs = [np.ascontiguousarray(c.offsets, dtype=np.uint64) if c.num_blocks else np.zeros(1, dtype=np.uint64) for c in containers]
    keep += stream_arrs + offs
    p_streams = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in stream_arrs])
    p_offs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in offs])
    lens = np.array([a.size for a in stream_arrs] or [0], dtype=np.uint64)
    totals = np.array([c.total for c in containers] or [0], dtype=np.uint32)
    bss = np.array([c.block_size for c in containers] or [0], dtype=np.uint32)
    nbs = np.array([c.num_blocks for c in containers] or [0], dtype=np.uint32)
    if dst_offsets is None:
        dst_offsets, buf_len = rc.layout([int(length) if length < (1 << 40) else 0 for _, _, length in requests])
    buf = np.full(buf_len, rc.GUARD, dtype=np.uint8)
    arr = np.zeros(max(len(requests), 1), dtype=[("offset", "<u8"), ("length", "<u8"), ("dst", "<u8"), ("stream", "<u4"), ("pad", "<u4")])
    for i, (s, off, length) in enumerate(requests):
        arr[i] = (off, length, buf.ctypes.data + dst_offsets[i], s, 0)
    status = np.full(max(len(requests), 1), 0x55, dtype=np.uint32)
    mbs = max_block_size or max(c.block_size for c in containers)
    emu_lib().emu_decompress_ranges(n, p_streams, lens.ctypes.data, p_offs, totals.ctypes.data, bss.ctypes.data, nbs.ctypes.data,
                                    arr.ctypes.data, len(requests), status.ctypes.data, mbs, slots, grid)
    return [int(x) for x in status[:len(requests)]], buf, dst_offsets


def check_ok(containers, requests, **kw):
    st, buf, offs = run(containers, requests, **kw)
    expected = [(offs[i], length, containers[s].plain[off:off + length]) for i, (s, off, length) in enumerate(requests)]
    assert st == [0] * len(requests), [(requests[i], x) for i, x in enumerate(st) if x != 0]
    assert rc.check_buffer(buf, expected) == []


@pytest.mark.parametrize("name", ["alice", "coding", "terror2"])
def test_ranges_goldens(name):
    c = rc.Container(golden_bytes(name + ".txt"), golden_bytes(name + ".snappy"))
    check_ok([c], [(0, o, n) for o, n in rc.boundary_ranges(c.total, c.block_size, seed=len(name))])


@pytest.mark.parametrize("bs,n", [(1, 300), (7, 2000), (64, 6000), (4096, 30000), (32768, 90000), (65535, 140000)])
def test_ranges_block_sizes_vs_oracle(bs, n):
    text = golden_bytes("plrabn12.txt")
    c = rc.Container(datagen.text_random_interleave(text, n, seed=bs), block_size=bs)
    check_ok([c], [(0, o, k) for o, k in rc.boundary_ranges(c.total, bs, seed=bs, random_count=8)])


def test_ranges_mixed_block_sizes_one_call():
    text = golden_bytes("plrabn12.txt")
    cs = [rc.Container(text[:700], block_size=7), rc.Container(text[:20000], block_size=4096), rc.Container(text[:80000], block_size=65535),
          rc.Container(datagen.periodic(3000, 13), block_size=64)]
    reqs = []
    for i, c in enumerate(cs):
        reqs += [(i, o, n) for o, n in rc.boundary_ranges(c.total, c.block_size, seed=i, random_count=3)]
    check_ok(cs, reqs)


def test_ranges_overlapping_into_separate_destinations():
    c = rc.Container(golden_bytes("terror2.txt"), block_size=4096)
    reqs = [(0, 1000, 9000), (0, 1000, 9000), (0, 4000, 200), (0, 3000, 5000), (0, 8191, 2), (0, 0, c.total)]
    check_ok([c], reqs)


def test_ranges_adjacent_rebuild_the_plaintext():
    """Adjacent ranges packed back to back into ONE buffer: together they are the plaintext, nothing around it is written."""
    c = rc.Container(golden_bytes("terror2.txt")[:50000], block_size=4096)
    rng = np.random.default_rng(5)
    cuts = sorted({0, c.total} | {int(x) for x in rng.integers(0, c.total, 14)} | {4096, 4097, 8191})
    reqs = [(0, a, b - a) for a, b in zip(cuts, cuts[1:])]
    base = 29
    st, buf, _ = run([c], reqs, dst_offsets=[base + a for a, _ in zip(cuts, cuts[1:])], buf_len=base + c.total + 31)
    assert st == [0] * len(reqs)
    assert rc.check_buffer(buf, [(base, c.total, c.plain)]) == []


def test_ranges_out_of_bounds_and_overflow_leave_dst_untouched():
    c = rc.Container(golden_bytes("coding.txt"), block_size=4096)
    big = (1 << 64) - 1
    reqs = [(0, c.total - 10, 11), (0, c.total + 1, 0), (0, big, 2), (0, 5, big), (1, 0, 10), (7, 0, 0), (0, 100, 50)]
    st, buf, offs = run([c], reqs, dst_offsets=[40 * i + 7 for i in range(len(reqs))], buf_len=40 * len(reqs) + 64)
    assert st == [rc.OUT_OF_BOUNDS] * 6 + [0]
    assert rc.check_buffer(buf, [(offs[6], 50, c.plain[100:150])]) == []


def test_ranges_damaged_block_is_invalid_only_where_touched():
    c = rc.Container(golden_bytes("terror2.txt")[:40000], block_size=4096)
    damaged = bytearray(c.stream)
    at = int(c.offsets[3])
    size = int.from_bytes(damaged[at:at + 4], "little")
    damaged[at:at + 4] = (size - 1).to_bytes(4, "little")          # block 3 now ends inside its last element
    bs = c.block_size
    reqs = [(0, 3 * bs + 10, 5), (0, 2 * bs, 2 * bs), (0, 0, 3 * bs), (0, 4 * bs, 3 * bs), (0, 3 * bs - 1, 1), (0, 4 * bs, 1),
            (0, 0, c.total), (0, 3 * bs, bs)]
    st, buf, offs = run([c], reqs, streams=[bytes(damaged)])
    touched = [True, True, False, False, False, False, True, True]
    assert st == [1 if t else 0 for t in touched], st
    expected = [(offs[i], n, "any" if touched[i] else c.plain[o:o + n]) for i, (_, o, n) in enumerate(reqs)]
    assert rc.check_buffer(buf, expected) == []


@pytest.mark.parametrize("slots,grid", [(1, 1), (1, 3), (2, 3)])
def test_ranges_small_scratch(slots, grid):
    c = rc.Container(golden_bytes("plrabn12.txt")[:30000], block_size=4096)
    check_ok([c], [(0, o, n) for o, n in rc.boundary_ranges(c.total, 4096, seed=9, random_count=4)], slots=slots, grid=grid)


def test_ranges_block_size_above_max_is_out_of_bounds():
    c = rc.Container(golden_bytes("plrabn12.txt")[:20000], block_size=4096)
    st, buf, offs = run([c], [(0, 10, 100), (0, 0, 0)], max_block_size=4095)
    assert st == [rc.OUT_OF_BOUNDS, 0]
    assert rc.check_buffer(buf, []) == []
