"""The emulator libraries of the four kernels that carry K1's parse besides the product kernels, built from
tests/emu/emu_k1_carriers.cpp: each carrier's own emulator source with emu_alias_stats added (snappy_kernels.hpp:
g_alias_stats).  lib(carrier) puts the library in the place of the one the carrier's binding loads, so that the binding's
calls and the helpers of the carrier's emulated test run the library whose statistics are read.  Test infrastructure only."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCES = {"raw": "emu_raw.cpp", "sz": "emu_sz.cpp", "update": "emu_update.cpp", "resize": "emu_resize.cpp"}
_LIBS = {}


def _binding(carrier):
    """(the module that holds the carrier's library in _LIB, its loader)"""
    if carrier == "raw":
        import emu_raw_lib as m
        return m, m.lib
    if carrier == "sz":
        import emu_sz_lib as m
        return m, m.lib
    if carrier == "update":
        import test_update_emulated as m
        return m, m.emu_lib
    import test_resize_emulated as m
    return m, m.emu_lib


def lib(carrier):
    if carrier not in _LIBS:
        module, loader = _binding(carrier)
        plain = loader()                      # built from every source it depends on, its entry points declared
        src = os.path.join(HERE, "emu", "emu_k1_carriers.cpp")
        out = os.path.join(HERE, "emu", "libsnappy_emu_k1_carrier_%s.so" % carrier)
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, plain._name)):
            tmp = out + f".{os.getpid()}.tmp"
            csrc = os.path.join(ROOT, "pim-compression_amd", "csrc")
            # -DSNAPPY_ABLATION: emu_runtime.cpp also drives the experiment kernel under csrc/ablation/ (as tests/emu_lib.py builds it)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSNAPPY_ABLATION", '-DK1_CARRIER_SOURCE="%s"' % SOURCES[carrier],
                                   "-I" + os.path.join(HERE, "emu"), "-I" + csrc, src, "-o", tmp])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        for name, fn in vars(plain).items():  # the entry points the binding declared, declared alike
            if isinstance(fn, ctypes._CFuncPtr):
                getattr(L, name).restype, getattr(L, name).argtypes = fn.restype, fn.argtypes
        module._LIB = _LIBS[carrier] = L
    return _LIBS[carrier]
