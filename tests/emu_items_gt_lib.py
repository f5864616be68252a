"""ctypes binding of tests/emu/emu_items_gt.cpp: the raw / .sz compress calls with K1's global-table wavefronts
(pim-compression_amd/csrc/snappy_items_gt.hpp) on the CPU wave emulator, in a library of its own.  Test infrastructure only."""
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
        src = os.path.join(HERE, "emu", "emu_items_gt.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_items_gt.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_raw.hpp", "snappy_crc32c.hpp",
                                             "snappy_sz.hpp", "snappy_items_gt.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        L.emu_items_gt_dst_fill.restype = ctypes.c_uint
        L.emu_items_gt_table_bytes.restype = ctypes.c_ulonglong
        L.emu_items_gt_compress.restype = ci
        L.emu_items_gt_compress.argtypes = [ci, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, u32, ci, ci, vp]
        _LIB = L
    return _LIB


class Batch(RawBatch):
    """items as emu_raw_lib.Batch: (src bytes, capacity[, flags[, src_len]]); result has the new calls' four words"""

    def __init__(self, items, spares=None):
        super().__init__(items)
        self.result = np.full(4, 0x77, dtype=np.uint32)
        self.spare = np.array(list(spares if spares is not None else [0] * self.n) + [0], dtype=np.uint32)


def junk_tables(grid, seed=1):
    """`grid` tables in the state a workspace is in that nobody initialised: random bytes"""
    words = grid * int(lib().emu_items_gt_table_bytes()) // 4
    return np.random.default_rng(seed).integers(0, 1 << 32, size=words, dtype=np.uint64).astype(np.uint32)


def compress(fmt, items, block_size, max_units, grid=3, form=3, cached=True, tables=None, spares=None):
    """fmt: "raw" or "sz".  -> (rc, Batch): rc 100 = a kernel wrote in front of a window.  Writes behind a window fault.
    tables: junk_tables(grid) by default; pass an array to run on what an earlier run left in it."""
    assert fmt in ("raw", "sz")
    b = Batch(items, spares)
    if tables is None:
        tables = junk_tables(grid)
    assert tables.dtype == np.uint32 and tables.nbytes >= grid * int(lib().emu_items_gt_table_bytes())
    rc = lib().emu_items_gt_compress(fmt == "sz", b.src.ctypes.data, b.real_len.ctypes.data, b.src_len.ctypes.data, b.capacity.ctypes.data,
                                     b.flags.ctypes.data, b.spare.ctypes.data, b.n, block_size, max_units, b.out.ctypes.data, b.out_len.ctypes.data,
                                     b.status.ctypes.data, b.result.ctypes.data, grid, form, 1 if cached else 0, tables.ctypes.data)
    return rc, b
