"""ctypes binding of tests/emu/emu_raw_check_split.cpp: the split check of raw Snappy streams
(csrc/snappy_raw_check_split.hpp) on the CPU wave emulator, in a library of its own.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None

FLAG_CLASS, FLAG_FALLBACK, CLASS_SPLIT = 3, 4, 2       # an item's flag word (csrc/snappy_raw_split.hpp)


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_raw_check_split.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_raw_check_split.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_raw.hpp",
                                             "snappy_check.hpp", "snappy_raw_split.hpp", "snappy_raw_check_split.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.emu_raw_check_split.restype = ctypes.c_int
        L.emu_raw_check_split.argtypes = [vp, vp, vp, vp, u32, u32, u64, vp, vp, vp, u32, vp, vp, vp, vp, u64]
        _LIB = L
    return _LIB


def segments_of(items, segment_bytes):
    """segments that hold every item of the batch"""
    return sum((len(it[0]) + segment_bytes - 1) // segment_bytes for it in items)


class Checked:
    pass


def check_split(items, segment_bytes=16384, max_segments=None, grid=3, trace=False):
    """items: list of src bytes, or (src bytes, flags, src_len); flags bit 0 = null src -> (rc, Checked): verdicts[i] = (status,
    out_len), result = the four result words.  rc 101 = a kernel wrote behind the scratch.  A limit left out holds the whole
    batch.  trace: also plan_flags[i] and step4_flags[i] (the item's flag word after step 1 and after step 4) and nodes[i] (one
    (entry, landing, output base) or None per segment, as step 3 left them; None unless the plan classed the item large
    inside the limit)."""
    items = [it if isinstance(it, tuple) else (it,) for it in items]
    n = len(items)
    keep = [np.frombuffer(it[0], dtype=np.uint8).copy() if len(it[0]) else np.zeros(1, dtype=np.uint8) for it in items]
    src = np.array([k.ctypes.data for k in keep] + [0], dtype=np.uint64)
    real_len = np.array([len(it[0]) for it in items] + [0], dtype=np.uint64)
    src_len = np.array([(it[2] if len(it) > 2 else len(it[0])) for it in items] + [0], dtype=np.uint64)
    flags = np.array([(it[1] if len(it) > 1 else 0) for it in items] + [0], dtype=np.uint32)
    out_len = np.full(n + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    status = np.full(n + 1, 0x55, dtype=np.uint32)
    result = np.full(5, 0x77, dtype=np.uint32)
    need = segments_of(items, segment_bytes)
    plan_flags, step4, count = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    nodes = np.zeros(3 * need + 3, np.uint32)
    rc = lib().emu_raw_check_split(src.ctypes.data, real_len.ctypes.data, src_len.ctypes.data, flags.ctypes.data, n, segment_bytes,
                                   need if max_segments is None else max_segments, out_len.ctypes.data, status.ctypes.data, result.ctypes.data, grid,
                                   plan_flags.ctypes.data if trace else None, step4.ctypes.data if trace else None,
                                   count.ctypes.data if trace else None, nodes.ctypes.data if trace else None, 3 * need)
    assert rc >= 0, "the trace's arrays are too small"
    assert int(result[4]) == 0x77 and int(status[n]) == 0x55 and int(out_len[n]) == 0x5A5A5A5A5A5A5A5A    # nothing behind the arrays
    c = Checked()
    c.verdicts = [(int(status[i]), int(out_len[i])) for i in range(n)]
    c.result = [int(x) for x in result[:4]]
    if trace:
        c.plan_flags, c.step4_flags = [int(x) for x in plan_flags[:n]], [int(x) for x in step4[:n]]
        c.nodes = [None] * n
        at = 0
        for i in range(n):
            nn = int(count[i])
            if nn:
                trip = nodes[at:at + 3 * nn].reshape(nn, 3)
                c.nodes[i] = [None if int(t[0]) == 0xffffffff else (int(t[0]), int(t[1]), int(t[2])) for t in trip]
            at += 3 * nn
    return rc, c
