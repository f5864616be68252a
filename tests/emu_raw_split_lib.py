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


def decompress_split(items, unit_len=65536, segment_bytes=65536, max_segments=None, max_units=None, grid=3):
    """items as emu_raw_lib.Batch takes them -> (rc, Batch); Batch.result holds the four result words.  rc 100 = a kernel wrote
    in front of a window.  Writes behind a window fault.  Limits left out hold the whole batch."""
    b = emu_raw_lib.Batch(items)
    b.result = np.full(5, 0x77, dtype=np.uint32)
    need_s, need_u = limits(items, unit_len, segment_bytes)
    rc = lib().emu_raw_decompress_split(b.src.ctypes.data, b.real_len.ctypes.data, b.src_len.ctypes.data, b.capacity.ctypes.data, b.flags.ctypes.data,
                                        b.n, unit_len, segment_bytes, need_s if max_segments is None else max_segments,
                                        need_u if max_units is None else max_units, b.out.ctypes.data, b.out_len.ctypes.data, b.status.ctypes.data,
                                        b.result.ctypes.data, grid)
    assert int(b.result[4]) == 0x77 and int(b.status[b.n]) == 0x55 and int(b.out_len[b.n]) == 0x5A5A5A5A5A5A5A5A    # nothing behind the arrays
    return rc, b
