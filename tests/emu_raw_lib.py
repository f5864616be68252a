"""ctypes binding of tests/emu/emu_raw.cpp: the raw-Snappy batch kernels on the CPU wave emulator, in a library of its own.
Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_raw.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_raw.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_raw.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        L.emu_raw_max_len.restype = ctypes.c_ulonglong
        L.emu_raw_dst_fill.restype = ctypes.c_uint
        L.emu_raw_decompress.restype = ctypes.c_int
        L.emu_raw_decompress.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, vp, u32]
        L.emu_raw_compress.restype = ctypes.c_int
        L.emu_raw_compress.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, u32, ctypes.c_int]
        _LIB = L
    return _LIB


class Batch:
    """items: list of (src bytes, capacity) or (src bytes, capacity, flags, src_len); flags bit 0 = null src, bit 1 = null dst;
    src_len overrides len(src) (for a null src)."""

    def __init__(self, items):
        n = len(items)
        self.n = n
        self.keep = [np.frombuffer(it[0], dtype=np.uint8).copy() if len(it[0]) else np.zeros(1, dtype=np.uint8) for it in items]
        self.src = np.array([k.ctypes.data for k in self.keep] + [0], dtype=np.uint64)
        self.real_len = np.array([len(it[0]) for it in items] + [0], dtype=np.uint64)
        self.src_len = np.array([(it[3] if len(it) > 3 else len(it[0])) for it in items] + [0], dtype=np.uint64)
        self.capacity = np.array([it[1] for it in items] + [0], dtype=np.uint64)
        self.flags = np.array([(it[2] if len(it) > 2 else 0) for it in items] + [0], dtype=np.uint32)
        self.outs = [np.zeros(max(int(it[1]), 1), dtype=np.uint8) for it in items]
        self.out = np.array([o.ctypes.data for o in self.outs] + [0], dtype=np.uint64)
        self.out_len = np.full(n + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        self.status = np.full(n + 1, 0x55, dtype=np.uint32)
        self.result = np.full(2, 0x77, dtype=np.uint32)

    def window(self, i):
        """the whole dst window of item i after the run (capacity bytes)"""
        return self.outs[i][:int(self.capacity[i])].tobytes()


def decompress(items, grid=3):
    """-> (rc, Batch): rc 100 = a kernel wrote in front of a window.  Writes behind a window fault."""
    b = Batch(items)
    rc = lib().emu_raw_decompress(b.src.ctypes.data, b.real_len.ctypes.data, b.src_len.ctypes.data, b.capacity.ctypes.data, b.flags.ctypes.data, b.n, b.out.ctypes.data,
                                  b.out_len.ctypes.data, b.status.ctypes.data, grid)
    return rc, b


def compress(items, block_size, max_fragments, grid=3, form=3):
    b = Batch(items)
    rc = lib().emu_raw_compress(b.src.ctypes.data, b.real_len.ctypes.data, b.src_len.ctypes.data, b.capacity.ctypes.data, b.flags.ctypes.data, b.n, block_size,
                                max_fragments, b.out.ctypes.data, b.out_len.ctypes.data, b.status.ctypes.data, b.result.ctypes.data, grid, form)
    return rc, b
