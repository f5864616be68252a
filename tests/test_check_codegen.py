"""CPU test of the generated code of the check kernels (pim-compression_amd/csrc/snappy_check.hpp): the three of them are in
the device code; none spills (private_segment_fixed_size 0); check_kernel and raw_check_kernel use no LDS at all -- the check
has no stage -- and stay within 64 VGPRs, eight wavefronts per SIMD, as K2 has; and their pointers, which come from
descriptors in memory (load_global_ptr), give global_* instructions, never flat_* ones."""
import os
import re
import subprocess

from conftest import ROOT

import __graft_entry__ as entry

KERNELS = ("check_plan_kernel", "check_kernel", "raw_check_kernel")


def _field(body, name):
    return int(re.search(r"^\s*\.amdhsa_" + name + r" (\d+)", body, re.M).group(1))


def test_check_kernels_are_present_lean_and_without_lds(tmp_path):
    src = os.path.join(ROOT, "pim-compression_amd", "csrc", "snappy_hip.hip")
    asm = tmp_path / "device.s"
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(asm)])
    text = asm.read_text()
    for name in KERNELS:
        m = re.search(r"^(_ZN10snappy_hip\d+" + name + r"E\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
        assert m, name
        body = m.group(2)
        assert _field(body, "private_segment_fixed_size") == 0, name
        assert re.findall(r"^\s*flat_\w+", body, re.M) == [], name
        assert re.findall(r"^\s*scratch_\w+", body, re.M) == [], name
        if name == "check_plan_kernel":
            continue
        assert _field(body, "group_segment_fixed_size") == 0, name
        assert re.findall(r"^\s*ds_(?:read|write|load|store)\w*", body, re.M) == [], name     # (ds_bpermute / ds_permute touch no LDS)
        assert _field(body, "next_free_vgpr") <= 64, name
        # the verdicts and the result words are the only stores: a handful, where K2 has dozens
        assert len(re.findall(r"^\s*global_store", body, re.M)) <= 4, name
        assert len(re.findall(r"^\s*global_load", body, re.M)) >= 10, name
        # The wavefront stays together from one draw to the next: the persistent loop (depth 1) holds the window loop (depth 2)
        # and nothing deeper.  Without the convergent operation that ends a trip the compiler sends the lanes that skip the
        # `lane == 0` part round a loop of their own -- the persistent loop inside another one, the window loop at depth 3 --
        # in which they read their own `drawn = 0` for ever.  The emulator cannot see this; the generated code shows it.
        assert "; wave barrier" in body, name
        assert "Depth=2" in body and "Depth=3" not in body, name
    # no kernel of the check counts as a K1 or K2 instantiation (tests/test_abi_symbols.py tells those by "_blocks_" and
    # "decompress_blocks_kernel")
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    mine = sorted(k for k in kernels if "check_" in k)
    assert len(mine) == len(KERNELS) and not any("_blocks_" in k for k in mine), mine
