"""ctypes binding of tests/emu/emu_k1_alias.cpp: K1 on the CPU wave emulator, in a library of its own that also exports the
second statistics array (snappy_kernels.hpp: g_alias_stats).  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None

# g_alias_stats by name (snappy_kernels.hpp)
ALIAS_STATS = ("entered", "cleared", "kept", "fallback_windows", "settle_cx", "settle_deep", "settle_partner_not_inserted",
               "settle_partner_inserted", "settle_saturated_only", "long_way_found_nothing")
# g_stream_stats entries of the stream form that the alias tests and tools read
WINDOWS_TAKEN, SETTLES, LONG_WAY = 0, 3, 6


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "emu_k1_alias.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_k1_alias.so")
        csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_runtime.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")] + \
            [os.path.join(csrc, f) for f in ("snappy_device_common.hpp", "snappy_kernels.hpp", "snappy_k1_stream.hpp")] + \
            [os.path.join(csrc, "ablation", f) for f in os.listdir(os.path.join(csrc, "ablation"))]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = out + f".{os.getpid()}.tmp"
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", "-I" + os.path.join(HERE, "emu"), "-I" + csrc,
                                   src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        L.emu_compress_variant.restype = ctypes.c_uint64
        L.emu_compress_variant.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
        L.emu_decompress.restype = ctypes.c_int
        L.emu_decompress.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        _LIB = L
    return _LIB


def compress(data, block_size, variant):
    """K1 + scan + gather of compress variant `variant` (tests/emu/emu_runtime.cpp: emu_compress_variant) -> the stream"""
    a = np.frombuffer(data, dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    n = len(data)
    nb = (n + block_size - 1) // block_size
    stride = (4 + 32 + block_size + block_size // 6 + 15) & ~15
    cap = 10 + nb * stride
    out = np.zeros(cap + 16, dtype=np.uint8)
    got = lib().emu_compress_variant(a.ctypes.data, n, block_size, out.ctypes.data, cap, variant)
    assert got > 0
    return out[:got].tobytes()


def decompress(stream, total_len, block_size, header_len):
    a = np.frombuffer(stream, dtype=np.uint8).copy()
    out = np.zeros(max(total_len, 1), dtype=np.uint8)
    st = lib().emu_decompress(a.ctypes.data, a.size, total_len, block_size, header_len, out.ctypes.data)
    return st, out[:total_len].tobytes()


def _read(fn):
    out = (ctypes.c_ulonglong * 16)()
    fn(out)
    return tuple(out)


def stream_stats():
    """g_stream_stats of this library (cleared by the read)"""
    return _read(lib().emu_stream_stats)


def alias_stats():
    """g_alias_stats (cleared by the read)"""
    return _read(lib().emu_alias_stats)
