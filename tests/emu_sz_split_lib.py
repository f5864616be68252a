"""ctypes binding of tests/emu/emu_sz_split.cpp: the split walk of .sz streams (csrc/snappy_sz_split.hpp) and the base call's
kernels on the CPU wave emulator, in a library of its own.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

from emu_sz_lib import Batch as SzBatch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_sz_split.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_sz_split.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_sz.cpp"), os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_raw.hpp", "snappy_crc32c.hpp",
                                             "snappy_sz.hpp", "snappy_sz_split.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.emu_sz_split_decompress.restype = ci
        L.emu_sz_split_decompress.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u64, u32, vp, vp, vp, vp, vp, u32, ci, vp, u64, vp, vp, vp]
        _LIB = L
    return _LIB


def decompress(items, max_chunks, segment_bytes, max_segments, flags=0, grid=3, tables=1):
    """items as emu_sz_lib.Batch.  segment_bytes 0: the base call's kernels (max_segments is ignored) -> (rc, Batch); the Batch
    also has result (4 words; the base call leaves [2] and [3] at their fill), records (the SzChunk records the call decoded
    from, 8 words each, as tuples), path_on and path_segs (per item the parallel walk proved: the segments on its path / all its
    segments; 0 otherwise).  rc 100 = a kernel wrote in front of a window, 101 = behind the scratch."""
    b = SzBatch(items)
    b.result = np.full(5, 0x77, dtype=np.uint32)
    room = max_chunks
    words = np.zeros(8 * room + 8, dtype=np.uint32)
    n_rec = np.zeros(1, dtype=np.uint32)
    path_on, path_segs = np.zeros(b.n + 1, dtype=np.uint32), np.zeros(b.n + 1, dtype=np.uint32)
    rc = lib().emu_sz_split_decompress(b.src.ctypes.data, b.real_len.ctypes.data, b.src_len.ctypes.data, b.capacity.ctypes.data, b.flags.ctypes.data,
                                       b.n, max_chunks, segment_bytes, max_segments, flags, b.out.ctypes.data, b.out_len.ctypes.data,
                                       b.status.ctypes.data, b.bad_chunk.ctypes.data, b.result.ctypes.data, grid, tables, words.ctypes.data, room,
                                       n_rec.ctypes.data, path_on.ctypes.data, path_segs.ctypes.data)
    # nothing behind the arrays' last entry
    assert int(b.result[4]) == 0x77 and int(b.status[b.n]) == 0x55 and int(b.bad_chunk[b.n]) == 0x66 and int(b.out_len[b.n]) == 0x5A5A5A5A5A5A5A5A
    n = min(int(n_rec[0]), room)
    b.records = [tuple(int(x) for x in words[8 * k:8 * k + 8]) for k in range(n)]
    b.path_on, b.path_segs = [int(x) for x in path_on[:b.n]], [int(x) for x in path_segs[:b.n]]
    return rc, b
