"""ctypes binding of tests/emu/emu_sz_ranges.cpp: the index and range kernels of .sz streams (csrc/snappy_sz_ranges.hpp) behind the
split walk's kernels on the CPU wave emulator, in a library of its own.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None
FILL = 0xEE


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_sz_ranges.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_sz_ranges.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_sz.cpp"), os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_raw.hpp", "snappy_crc32c.hpp",
                                             "snappy_sz.hpp", "snappy_sz_split.hpp", "snappy_ranges.hpp", "snappy_sz_ranges.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.emu_sz_ranges.restype = ci
        L.emu_sz_ranges.argtypes = [vp, vp, vp, vp, u32, u32, u32, u64, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, u32, u32]
        _LIB = L
    return _LIB


class Run:
    pass


def run(streams, max_chunks, segment_bytes, max_segments, ranges, flags=0, grid=3, slots=None, edits=(), null_src=()):
    """streams: [bytes]; ranges: [(stream, offset, length, null_dst)]; edits: [(record number, 8 words)] applied to the index before
    the ranges run; null_src: item numbers whose src is null.  -> (rc, Run) with idx_status, result (4 words), records (tuples of 8
    words), n_records (what the batch needs), descs (tuples: src is the item's, src_len, first chunk, num_chunks, total_len),
    status, bad_chunk and window(r) per range.  rc 100 = a kernel wrote in front of a window, 101 = behind a scratch."""
    n = len(streams)
    keep = [np.frombuffer(s, dtype=np.uint8).copy() if len(s) else np.zeros(1, dtype=np.uint8) for s in streams]
    src = np.array([k.ctypes.data for k in keep] + [0], dtype=np.uint64)
    lens = np.array([len(s) for s in streams] + [0], dtype=np.uint64)
    iflags = np.array([1 if i in null_src else 0 for i in range(n)] + [0], dtype=np.uint32)
    words = np.zeros(8 * max_chunks + 8, dtype=np.uint32)
    n_rec = np.zeros(1, dtype=np.uint32)
    descs = np.zeros(5 * n + 5, dtype=np.uint64)
    o = Run()
    o.idx_status = np.full(n + 1, 0x55, dtype=np.uint32)
    o.result = np.full(5, 0x77, dtype=np.uint32)
    e_at = np.array([e[0] for e in edits] + [0], dtype=np.uint32)
    e_words = np.array([w for e in edits for w in e[1]] + [0] * 8, dtype=np.uint32)
    m = len(ranges)
    r_stream = np.array([r[0] for r in ranges] + [0], dtype=np.uint32)
    r_off = np.array([r[1] for r in ranges] + [0], dtype=np.uint64)
    r_len = np.array([r[2] for r in ranges] + [0], dtype=np.uint64)
    r_flags = np.array([1 if r[3] else 0 for r in ranges] + [0], dtype=np.uint32)
    outs = [np.full(max(r[2] if r[2] <= 1 << 30 else 0, 1), 0x11, dtype=np.uint8) for r in ranges]
    out = np.array([x.ctypes.data for x in outs] + [0], dtype=np.uint64)
    o.status = np.full(m + 1, 0x55, dtype=np.uint32)
    o.bad_chunk = np.full(m + 1, 0x66, dtype=np.uint32)
    rc = lib().emu_sz_ranges(src.ctypes.data, lens.ctypes.data, lens.ctypes.data, iflags.ctypes.data, n, max_chunks, segment_bytes, max_segments,
                             words.ctypes.data, n_rec.ctypes.data, descs.ctypes.data, o.idx_status.ctypes.data, o.result.ctypes.data, len(edits),
                             e_at.ctypes.data, e_words.ctypes.data, r_stream.ctypes.data, r_off.ctypes.data, r_len.ctypes.data, r_flags.ctypes.data, m, n,
                             flags, out.ctypes.data, o.status.ctypes.data, o.bad_chunk.ctypes.data, grid, slots if slots is not None else grid)
    # nothing behind the arrays' last entry
    assert int(o.result[4]) == 0x77 and int(o.idx_status[n]) == 0x55 and int(o.status[m]) == 0x55 and int(o.bad_chunk[m]) == 0x66
    o.n_records = int(n_rec[0])
    k = min(o.n_records, max_chunks)
    o.records = [tuple(int(x) for x in words[8 * j:8 * j + 8]) for j in range(k)]
    o.descs = [tuple(int(x) for x in descs[5 * i:5 * i + 5]) for i in range(n)]
    o.window = lambda r: bytes(outs[r][:ranges[r][2]]) if ranges[r][2] <= 1 << 30 else b""
    return rc, o
