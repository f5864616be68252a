"""CPU test of the generated code of the split decode (pim-compression_amd/csrc/snappy_raw_split.hpp): its six kernels are in
the device code; none spills or uses scratch memory (private_segment_fixed_size 0, no scratch_* instruction); their pointers,
which come from items in memory (load_global_ptr), give global_* instructions, never flat_* ones -- the unit and serial kernels
run K2's decoder, which relies on global_* operations of one wavefront completing in issue order; the persistent ones keep
their wavefront together from one draw to the next; and every kernel the library had before is, instruction for instruction,
what tools/kernel_asm_diff.py finds in the parent commit's device code."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import __graft_entry__ as entry

KERNELS = ("raw_split_plan_kernel", "raw_split_walk_kernel", "raw_split_resolve_kernel", "raw_split_cuts_kernel", "raw_split_units_kernel",
           "raw_split_serial_kernel")
PERSISTENT = KERNELS[1:2] + KERNELS[3:]
HIP = os.path.join("pim-compression_amd", "csrc", "snappy_hip.hip")


def _compile(src, out):
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(out)])


def _field(body, name):
    return int(re.search(r"^\s*\.amdhsa_" + name + r" (\d+)", body, re.M).group(1))


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("split_codegen") / "device.s"
    _compile(os.path.join(ROOT, HIP), out)
    return out


def test_split_kernels_are_present_global_only_and_without_scratch(device_asm):
    text = device_asm.read_text()
    for name in KERNELS:
        m = re.search(r"^(_ZN10snappy_hip\d+" + name + r"E\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
        assert m, name
        body = m.group(2)
        assert _field(body, "private_segment_fixed_size") == 0, name
        assert re.findall(r"^\s*flat_\w+", body, re.M) == [], name
        assert re.findall(r"^\s*scratch_\w+", body, re.M) == [], name
        assert len(re.findall(r"^\s*global_(?:load|store|atomic)", body, re.M)) >= 5, name
        assert _field(body, "next_free_vgpr") <= 64 or name == "raw_split_plan_kernel", name      # eight wavefronts per SIMD, as K2
        if name in PERSISTENT:
            assert "; wave barrier" in body, name        # (see tests/test_check_codegen.py: the trip ends in a convergent operation)
        if name in ("raw_split_walk_kernel", "raw_split_resolve_kernel", "raw_split_cuts_kernel"):
            assert _field(body, "group_segment_fixed_size") == 0, name                            # no stage: nothing is decoded here
            assert re.findall(r"^\s*ds_(?:read|write|load|store)\w*", body, re.M) == [], name
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    mine = sorted(k for k in kernels if "raw_split_" in k)
    assert len(mine) == len(KERNELS) and not any("_blocks_" in k for k in mine), mine


def test_kernels_of_the_parent_commit_are_unchanged(device_asm, tmp_path):
    """The parent commit's tree is taken from git (the parent of the commit that added snappy_raw_split.hpp), compiled the same
    way and compared kernel by kernel.  A later change that alters one of those kernels on purpose retires this test."""
    git = ["git", "-C", ROOT]
    if subprocess.run(git + ["rev-parse", "--git-dir"], capture_output=True).returncode != 0:
        pytest.skip("not a git checkout: there is no parent commit to compare with")
    added = subprocess.run(git + ["log", "--diff-filter=A", "--format=%H", "--", "pim-compression_amd/csrc/snappy_raw_split.hpp"],
                           capture_output=True, text=True, check=True).stdout.split()
    parent = (added[-1] + "^") if added else "HEAD"       # (not committed yet: HEAD is the parent)
    if subprocess.run(git + ["rev-parse", "--verify", "--quiet", parent + "^{commit}"], capture_output=True).returncode != 0:
        pytest.skip("the history does not reach the parent commit")
    tree = tmp_path / "parent"
    tree.mkdir()
    tar = subprocess.run(git + ["archive", parent, "pim-compression_amd/csrc", "include"], capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", str(tree)], input=tar, check=True)
    before = tmp_path / "before.s"
    _compile(str(tree / HIP), before)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_asm_diff.py"), str(before), str(device_asm)], capture_output=True, text=True)
    lines = out.stdout.split("\n")
    assert out.returncode == 0 and not [ln for ln in lines if ln.startswith("DIFF")], [ln for ln in lines if not ln.startswith("SAME")]
    assert sum(ln.startswith("SAME") for ln in lines) >= 20 and sum(ln.startswith("NEW") for ln in lines) >= len(KERNELS)
