"""ctypes binding of tests/emu/emu_sz.cpp: the .sz and CRC-32C kernels on the CPU wave emulator, in a library of its own.
Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

from emu_raw_lib import Batch as RawBatch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_sz.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_sz.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_raw.hpp", "snappy_crc32c.hpp",
                                             "snappy_sz.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        L.emu_sz_dst_fill.restype = ctypes.c_uint
        L.emu_sz_crc_mask.restype = ctypes.c_uint
        L.emu_sz_crc_mask.argtypes = [ctypes.c_uint]
        L.emu_gf_mul.restype = ctypes.c_uint
        L.emu_gf_mul.argtypes = [ctypes.c_uint, ctypes.c_uint]
        L.emu_x_pow_words.restype = ctypes.c_uint
        L.emu_x_pow_words.argtypes = [ctypes.c_uint]
        L.emu_crc32c_batch.restype = ci
        L.emu_crc32c_batch.argtypes = [vp, vp, vp, u32, vp, u32, ci]
        L.emu_sz_decompress.restype = ci
        L.emu_sz_decompress.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, u32, ci]
        L.emu_sz_compress.restype = ci
        L.emu_sz_compress.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, u32, ci, ci]
        _LIB = L
    return _LIB


class Batch(RawBatch):
    """items as emu_raw_lib.Batch: (src bytes, capacity[, flags[, src_len]]); adds bad_chunk"""

    def __init__(self, items):
        super().__init__(items)
        self.bad_chunk = np.full(self.n + 1, 0x66, dtype=np.uint32)


def crc32c_batch(datas, pads=None, grid=3, tables=1):
    """-> list of CRCs; pads[i] bytes lie between item i's end and the inaccessible page (default 0)"""
    n = len(datas)
    keep = [np.frombuffer(d, dtype=np.uint8).copy() if len(d) else np.zeros(1, dtype=np.uint8) for d in datas]
    src = np.array([k.ctypes.data for k in keep] + [0], dtype=np.uint64)
    lens = np.array([len(d) for d in datas] + [0], dtype=np.uint64)
    pad = np.array(list(pads if pads is not None else [0] * n) + [0], dtype=np.uint32)
    crc = np.full(n + 1, 0x77777777, dtype=np.uint32)
    lib().emu_crc32c_batch(src.ctypes.data, lens.ctypes.data, pad.ctypes.data, n, crc.ctypes.data, grid, tables)
    assert int(crc[n]) == 0x77777777
    return [int(c) for c in crc[:n]]


def decompress(items, max_chunks, flags=0, grid=3, tables=1):
    """-> (rc, Batch): rc 100 = a kernel wrote in front of a window.  Writes behind a window fault."""
    b = Batch(items)
    rc = lib().emu_sz_decompress(b.src.ctypes.data, b.real_len.ctypes.data, b.src_len.ctypes.data, b.capacity.ctypes.data, b.flags.ctypes.data, b.n,
                                 max_chunks, flags, b.out.ctypes.data, b.out_len.ctypes.data, b.status.ctypes.data, b.bad_chunk.ctypes.data,
                                 b.result.ctypes.data, grid, tables)
    return rc, b


def compress(items, chunk_len, max_chunks, grid=3, form=3, tables=1):
    b = Batch(items)
    rc = lib().emu_sz_compress(b.src.ctypes.data, b.real_len.ctypes.data, b.src_len.ctypes.data, b.capacity.ctypes.data, b.flags.ctypes.data, b.n, chunk_len,
                               max_chunks, b.out.ctypes.data, b.out_len.ctypes.data, b.status.ctypes.data, b.result.ctypes.data, grid, form, tables)
    return rc, b
