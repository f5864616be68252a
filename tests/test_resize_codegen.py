"""CPU test of the generated code of the resize kernels (pim-compression_amd/csrc/snappy_resize.hpp): every one of them is in
the device code, and none holds a flat_* instruction.  The recompress kernel runs K2's decoder and K1's parse, which rely on
global_* operations of one wavefront completing in issue order (tests/test_abi_symbols.py); its pointers come from the
descriptor and the segments in memory (load_global_ptr), so the check is made on the code that comes out."""
import os
import re
import subprocess

from conftest import ROOT

import __graft_entry__ as entry

KERNELS = (("resize_mark_kernel", 3), ("resize_plan_kernel", 3), ("resize_recompress_kernelILi2E", 20), ("resize_recompress_kernelILi3E", 20))


def test_resize_kernels_are_present_and_use_global_not_flat_instructions(tmp_path):
    src = os.path.join(ROOT, "pim-compression_amd", "csrc", "snappy_hip.hip")
    asm = tmp_path / "device.s"
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(asm)])
    text = asm.read_text()
    for name, least in KERNELS:
        m = re.search(r"^(_ZN10snappy_hip\d+" + name + r"\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
        assert m, name
        assert re.findall(r"^\s*flat_\w+", m.group(2), re.M) == [], name
        assert len(re.findall(r"^\s*global_(?:load|store|atomic)", m.group(2), re.M)) >= least, name
    # no kernel of the resize counts as a K1 instantiation (tests/test_abi_symbols.py tells those by "_blocks_")
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    mine = sorted(k for k in kernels if "resize_" in k)
    assert len(mine) == len(KERNELS) and not any("_blocks_" in k for k in mine), mine
