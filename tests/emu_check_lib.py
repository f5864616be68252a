"""ctypes binding of tests/emu/emu_check.cpp: the check kernels (csrc/snappy_check.hpp) on the CPU wave emulator, in a library
of its own.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None

OK, INVALID, OUT_OF_BOUNDS = 0, 1, 2
NONE = 0xffffffff


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_check.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_check.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_raw.hpp",
                                             "snappy_check.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.emu_check_result_junk.restype = ctypes.c_uint
        L.emu_check_status_junk.restype = ctypes.c_uint
        L.emu_check_blocks.restype = ctypes.c_int
        L.emu_check_blocks.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, ctypes.c_int, vp, vp, vp, vp, u32]
        L.emu_check_block.restype = ctypes.c_int
        L.emu_check_block.argtypes = [vp, u64, u64, u32]
        L.emu_raw_check.restype = None
        L.emu_raw_check.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32]
        _LIB = L
    return _LIB


def _bytes_array(b):
    return np.frombuffer(b, dtype=np.uint8).copy() if len(b) else np.zeros(1, dtype=np.uint8)


def check_block(stream, at, out_len):
    """ONE block (size word at stream[at]) checked alone for an output of out_len bytes -> status; 100 + x: the container's
    result words disagree with the block's status.  A read behind the stream faults: call from a child process."""
    a = _bytes_array(stream)
    return lib().emu_check_block(a.ctypes.data, len(stream), at, out_len)


class Container:
    """One descriptor of a check call.  num_blocks / block_size / stream_len are what the descriptor claims; status_words is the
    size of the status array the test hands over (default: the claimed num_blocks)."""

    def __init__(self, stream, offsets, total_len, block_size, num_blocks=None, stream_len=None, flags=0, status_words=None):
        self.stream = stream
        self.offsets = list(offsets)
        self.total_len = total_len
        self.block_size = block_size
        self.num_blocks = len(self.offsets) if num_blocks is None else num_blocks
        self.stream_len = len(stream) if stream_len is None else stream_len
        self.flags = flags
        self.status_words = len(self.offsets) if status_words is None else status_words


def check_blocks(containers, status_mode=2, grid=3):
    """-> (rc, results [count][4], statuses: list of per-container lists as the arrays hold them afterwards).
    status_mode 0: no status array; 1: an array of null pointers; 2: every container's array given."""
    n = len(containers)
    keep = [_bytes_array(c.stream) for c in containers]
    offs = [np.array(c.offsets + [0], dtype=np.uint64) for c in containers]
    ptr = lambda arrs: np.array([a.ctypes.data for a in arrs] + [0], dtype=np.uint64)   # noqa: E731
    u64 = lambda xs: np.array(list(xs) + [0], dtype=np.uint64)                           # noqa: E731
    u32 = lambda xs: np.array(list(xs) + [0], dtype=np.uint32)                           # noqa: E731
    stream_p, offs_p = ptr(keep), ptr(offs)
    real_len, stream_len = u64(len(c.stream) for c in containers), u64(c.stream_len for c in containers)
    total_len, block_size = u32(c.total_len for c in containers), u32(c.block_size for c in containers)
    num_blocks, flags = u32(c.num_blocks for c in containers), u32(c.flags for c in containers)
    words = u32(c.status_words for c in containers)
    at = u64(np.concatenate([[0], np.cumsum(words[:n])])[:n].tolist())
    status = np.full(int(words[:n].sum()) + 1, 0x11111111, dtype=np.uint32)
    results = np.full(4 * n + 1, 0x22222222, dtype=np.uint32)
    rc = lib().emu_check_blocks(stream_p.ctypes.data, real_len.ctypes.data, stream_len.ctypes.data, offs_p.ctypes.data, total_len.ctypes.data,
                                block_size.ctypes.data, num_blocks.ctypes.data, flags.ctypes.data, n, status_mode, words.ctypes.data, at.ctypes.data,
                                status.ctypes.data, results.ctypes.data, grid)
    res = [[int(x) for x in results[4 * i:4 * i + 4]] for i in range(n)]
    sts = [[int(x) for x in status[int(at[i]):int(at[i]) + int(words[i])]] for i in range(n)]
    return rc, res, sts


def raw_check(items, grid=3):
    """items: list of src bytes, or (src bytes, flags, src_len); flags bit 0 = null src -> list of (status, out_len); the words
    behind the arrays' last entries are asserted untouched."""
    items = [it if isinstance(it, tuple) else (it,) for it in items]
    n = len(items)
    keep = [_bytes_array(it[0]) for it in items]
    src = np.array([k.ctypes.data for k in keep] + [0], dtype=np.uint64)
    real_len = np.array([len(it[0]) for it in items] + [0], dtype=np.uint64)
    src_len = np.array([(it[2] if len(it) > 2 else len(it[0])) for it in items] + [0], dtype=np.uint64)
    flags = np.array([(it[1] if len(it) > 1 else 0) for it in items] + [0], dtype=np.uint32)
    out_len = np.full(n + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    status = np.full(n + 1, 0x55, dtype=np.uint32)
    lib().emu_raw_check(src.ctypes.data, real_len.ctypes.data, src_len.ctypes.data, flags.ctypes.data, n, out_len.ctypes.data, status.ctypes.data, grid)
    assert int(status[n]) == 0x55 and int(out_len[n]) == 0x5A5A5A5A5A5A5A5A
    return [(int(status[i]), int(out_len[i])) for i in range(n)]


def fold(statuses):
    """the four result words of a well-formed container from its per-block statuses"""
    bad = [b for b, st in enumerate(statuses) if st != OK]
    return [INVALID if bad else OK, len(bad), bad[0] if bad else NONE, 0]
