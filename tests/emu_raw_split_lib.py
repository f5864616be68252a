"""ctypes binding of tests/emu/emu_raw_split.cpp: the split decode of raw Snappy streams (csrc/snappy_raw_split.hpp) on the CPU
wave emulator, in a library of its own.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import emu_raw_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_raw_split.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_raw_split.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_raw.hpp",
                                             "snappy_raw_split.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.emu_raw_split_dst_fill.restype = ctypes.c_uint
        L.emu_raw_decompress_split.restype = ctypes.c_int
        L.emu_raw_decompress_split.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u64, u64, vp, vp, vp, vp, u32]
        L.emu_raw_decompress_split_traced.restype = ctypes.c_int
        L.emu_raw_decompress_split_traced.argtypes = L.emu_raw_decompress_split.argtypes + [vp, vp, vp, vp, u64, vp, u64]
        _LIB = L
    return _LIB


def limits(items, unit_len, segment_bytes):
    """(segments, units) that hold every item of the batch"""
    import raw_cases
    segs = units = 0
    for it in items:
        h = raw_cases.header_parses(it[0])
        segs += (len(it[0]) + segment_bytes - 1) // segment_bytes
        units += (h[0] + unit_len - 1) // unit_len if h and h[0] <= raw_cases.RAW_MAX_LEN else 0
    return segs, units


FLAG_CLASS, FLAG_FALLBACK, CLASS_SPLIT = 3, 4, 2       # an item's flag word (csrc/snappy_raw_split.hpp)


def decompress_split(items, unit_len=65536, segment_bytes=65536, max_segments=None, max_units=None, grid=3, trace=False):
    """items as emu_raw_lib.Batch takes them -> (rc, Batch); Batch.result holds the four result words.  rc 100 = a kernel wrote
    in front of a window, 101 = behind the scratch.  Writes behind a window fault.  Limits left out hold the whole batch.
    trace: the Batch also gets what steps 1-4 left in the scratch: plan_flags[i] and flags[i] (the item's flag word after step
    1 and after step 4), cuts[i] (its units + 1 cuts) and nodes[i] (one (entry, landing, output base) or None per segment); the
    last two are None unless the plan classed the item split inside the limits."""
    b = emu_raw_lib.Batch(items)
    b.result = np.full(5, 0x77, dtype=np.uint32)
    need_s, need_u = limits(items, unit_len, segment_bytes)
    if trace:
        n = b.n
        plan_flags, flags, count = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(2 * n + 2, np.uint32)
        cuts, nodes = np.zeros(need_u + n + 1, np.uint32), np.zeros(3 * need_s + 3, np.uint32)
        rc = lib().emu_raw_decompress_split_traced(
            b.src.ctypes.data, b.real_len.ctypes.data, b.src_len.ctypes.data, b.capacity.ctypes.data, b.flags.ctypes.data, n, unit_len, segment_bytes,
            need_s if max_segments is None else max_segments, need_u if max_units is None else max_units, b.out.ctypes.data, b.out_len.ctypes.data,
            b.status.ctypes.data, b.result.ctypes.data, grid, plan_flags.ctypes.data, flags.ctypes.data, count.ctypes.data, cuts.ctypes.data,
            need_u + n, nodes.ctypes.data, 3 * need_s)
        assert rc >= 0, "the trace's arrays are too small"
        b.plan_flags, b.step4_flags = [int(x) for x in plan_flags[:n]], [int(x) for x in flags[:n]]
        b.cuts, b.nodes = [None] * n, [None] * n
        c_at = n_at = 0
        for i in range(n):
            nc, nn = int(count[2 * i]), int(count[2 * i + 1])
            if nc:
                b.cuts[i] = [int(x) for x in cuts[c_at:c_at + nc]]
                trip = nodes[n_at:n_at + 3 * nn].reshape(nn, 3)
                b.nodes[i] = [None if int(t[0]) == 0xffffffff else (int(t[0]), int(t[1]), int(t[2])) for t in trip]
            c_at += nc
            n_at += 3 * nn
        assert int(b.result[4]) == 0x77 and int(b.status[b.n]) == 0x55 and int(b.out_len[b.n]) == 0x5A5A5A5A5A5A5A5A
        return rc, b
    rc = lib().emu_raw_decompress_split(b.src.ctypes.data, b.real_len.ctypes.data, b.src_len.ctypes.data, b.capacity.ctypes.data, b.flags.ctypes.data,
                                        b.n, unit_len, segment_bytes, need_s if max_segments is None else max_segments,
                                        need_u if max_units is None else max_units, b.out.ctypes.data, b.out_len.ctypes.data, b.status.ctypes.data,
                                        b.result.ctypes.data, grid)
    assert int(b.result[4]) == 0x77 and int(b.status[b.n]) == 0x55 and int(b.out_len[b.n]) == 0x5A5A5A5A5A5A5A5A    # nothing behind the arrays
    return rc, b
