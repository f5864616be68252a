"""CPU tests of the device pieces every kernel header shares (pim-compression_amd/csrc/snappy_device_common.hpp): the UNMODIFIED
functions on the lockstep wave emulator, each driven alone by tests/emu/emu_common.cpp and held to a numpy model at the edges
their callers reach only by accident."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import to_raw_snappy as trs   # noqa: E402

GUARD = 0xEE
_LIB = None


def emu_lib():
    """tests/emu/emu_common.cpp in a library of its own (the emulator runtime + the shared pieces)."""
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_common.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_common.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        L.emu_common_scan.restype = None
        L.emu_common_scan.argtypes = [vp, u32, vp, vp]
        for f in (L.emu_common_workgroup_copy, L.emu_common_wave_copy):
            f.restype = None
            f.argtypes = [vp, vp, u32]
        L.emu_common_prefix_owner.restype = None
        L.emu_common_prefix_owner.argtypes = [vp, u32, vp, u32, vp, ctypes.c_int]
        L.emu_common_varint.restype = u32
        L.emu_common_varint.argtypes = [u32, vp, vp]
        _LIB = L
    return _LIB


# ---- workgroup_exclusive_scan ----
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2500])
def test_workgroup_scan_matches_cumsum(count):
    """Small values with 2^33 at every 7th element and at the last one of every wavefront and of every trip: the sums pass 2^32
    inside a wavefront, in the sums of the wavefronts and in the carry from trip to trip."""
    rng = np.random.default_rng(count)
    values = rng.integers(0, 1 << 20, max(count, 1)).astype(np.uint64)
    values[::7] = 1 << 33
    values[63::64] = 1 << 33
    values = values[:count]
    buf = np.concatenate([values, np.zeros(1, dtype=np.uint64)])              # (never an empty array's pointer)
    prefix = np.full(count + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    total = np.full(1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    emu_lib().emu_common_scan(buf.ctypes.data, count, prefix.ctypes.data, total.ctypes.data)
    inclusive = np.cumsum(values, dtype=np.uint64)
    assert np.array_equal(prefix[:count], inclusive - values)
    assert int(total[0]) == (int(inclusive[-1]) if count else 0)
    assert int(prefix[count]) == 0x5A5A5A5A5A5A5A5A                           # nothing behind the last element
    if count > 1:
        assert int(total[0]) > 1 << 32


# ---- workgroup_copy, wave_copy ----
COPY_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097, 4111]


@pytest.mark.parametrize("length", COPY_LENGTHS)
@pytest.mark.parametrize("kind", ["workgroup_copy", "wave_copy"])
def test_copies_keep_their_bounds(kind, length):
    """Every destination misalignment 0..15 against source misalignments 0, 1, 4, 15: the payload arrives and the 64 guard
    bytes on either side of it (and everything else around it) stay as they were."""
    copy = getattr(emu_lib(), "emu_common_" + kind)
    payload = np.random.default_rng(length).integers(0, 256, length + 32, dtype=np.uint8)
    payload[payload == GUARD] = 0x11                                          # (a missing byte must not look copied)
    src_buf = np.zeros(length + 64, dtype=np.uint8)
    src_base = (-src_buf.ctypes.data) % 16
    dst_buf = np.empty(64 + 16 + length + 64 + 16, dtype=np.uint8)
    dst_base = (-dst_buf.ctypes.data) % 16 + 64                               # 16-byte aligned, 64 guard bytes in front
    for src_mis in (0, 1, 4, 15):
        s = src_base + src_mis
        src_buf[:] = 0x77
        src_buf[s:s + length] = payload[:length]
        for dst_mis in range(16):
            d = dst_base + dst_mis
            assert (dst_buf.ctypes.data + d) % 16 == dst_mis and (src_buf.ctypes.data + s) % 16 == src_mis
            dst_buf[:] = GUARD
            copy(dst_buf.ctypes.data + d, src_buf.ctypes.data + s, length)
            assert np.array_equal(dst_buf[d:d + length], payload[:length]), (src_mis, dst_mis)
            assert (dst_buf[:d] == GUARD).all() and (dst_buf[d + length:] == GUARD).all(), (src_mis, dst_mis)


# ---- prefix_owner ----
@pytest.mark.parametrize("vector_loads", [0, 1], ids=["plain", "uld64"])      # both ways of reading the prefix
@pytest.mark.parametrize("counts", [
    [5],
    [0, 0, 3, 0, 1, 0, 0, 2, 5, 0],                  # owners of no work in front, in runs between the others and at the end
    [1] * 9,
    [0] * 6 + [1],
    [2, 0, 0, 0, 0, 0, 0, 2],
    [3, 1 << 32, 0, 7],                              # the prefix is 64 bits wide: entries beyond 2^32 own nothing a u32 can name
    list(np.random.default_rng(7).integers(0, 3, 200)),
], ids=["one", "runs", "ones", "last", "ends", "wide", "random200"])
def test_prefix_owner_matches_searchsorted(counts, vector_loads):
    counts = np.array(counts, dtype=np.uint64)
    inclusive = np.cumsum(counts, dtype=np.uint64)
    prefix = np.concatenate([inclusive - counts, inclusive[-1:]])            # [count] = all the work, as the planners leave it
    total = min(int(inclusive[-1]), 64)
    # every boundary (the first and the last work item of every owner) and everything between, where there is little
    p = sorted({x for b in prefix[:-1] for x in (int(b) - 1, int(b), int(b) + 1) if 0 <= x < min(int(inclusive[-1]), 1 << 32)} | set(range(total)))
    p = np.array(p, dtype=np.uint32)
    owner = np.full(len(p), 0x55555555, dtype=np.uint32)
    emu_lib().emu_common_prefix_owner(prefix.ctypes.data, len(counts), p.ctypes.data, len(p), owner.ctypes.data, vector_loads)
    expect = np.searchsorted(prefix[:-1], p.astype(np.uint64), "right") - 1
    assert np.array_equal(owner, expect.astype(np.uint32))
    assert (counts[owner] > 0).all()                                         # the owner of a work item has work


# ---- varints ----
@pytest.mark.parametrize("v", [0, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, (1 << 32) - 1])
def test_varints_match_the_converter(v):
    out = np.full(8, GUARD, dtype=np.uint8)
    n = np.zeros(1, dtype=np.uint32)
    put = emu_lib().emu_common_varint(v, out.ctypes.data, n.ctypes.data)
    expect = bytes(trs.varint(v))
    assert put == len(expect) == int(n[0])
    assert out[:put].tobytes() == expect and (out[put:] == GUARD).all()
