"""ctypes binding of tests/emu/emu_k2_wide.cpp: the wide block decoder (csrc/snappy_k2_wide.hpp) on the CPU wave emulator, in a
library of its own.  Test infrastructure only."""
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
        src = os.path.join(HERE, "emu", "emu_k2_wide.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_k2_wide.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp", "snappy_k2_wide.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.emu_k2_wide.restype = ctypes.c_int
        L.emu_k2_wide.argtypes = [vp, u64, vp, u64, u32, u32, u32, vp, vp, vp]
        L.emu_k2_wide_max_csz.restype = ctypes.c_uint
        L.emu_k2_wide_lds_bytes.restype = ctypes.c_uint
        _LIB = L
    return _LIB


def max_csz():
    return int(lib().emu_k2_wide_max_csz())


def decompress_wide(stream, offsets, total_len, block_size, waves=16, grid=1):
    """k2_wide_kernel over the blocks at `offsets` of one container, the output exactly total_len bytes between inaccessible
    pages -> (rc, statuses, bytes, the four result words); rc 100: a write in front of the window.  A write behind it or a read
    behind the stream faults: call from a child process."""
    a = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, dtype=np.uint8)
    offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
    nb = (total_len + block_size - 1) // block_size
    assert len(offs) == nb
    out = np.zeros(max(total_len, 1), dtype=np.uint8)
    status = np.full(nb + 1, 0x55, dtype=np.uint32)
    result = np.full(5, 0x77, dtype=np.uint32)
    rc = lib().emu_k2_wide(a.ctypes.data, len(stream), offs.ctypes.data, total_len, block_size, waves, grid, out.ctypes.data, status.ctypes.data,
                           result.ctypes.data)
    assert int(status[nb]) == 0x55 and int(result[4]) == 0x77                  # nothing behind the arrays
    return rc, [int(x) for x in status[:nb]], out[:total_len].tobytes(), [int(x) for x in result[:4]]


def decompress_block_wide(stream, at, out_len, waves=16):
    """ONE block decoded alone (as emu_lib.decompress_block gives it to K2) -> (status, bytes, result words)"""
    rc, st, out, res = decompress_wide(stream, [at], out_len, out_len, waves, 1)
    return (rc if rc else st[0]), out, res
