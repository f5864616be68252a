"""CPU test of the generated code of the wide block decoder (pim-compression_amd/csrc/snappy_k2_wide.hpp): k2_wide_kernel is in
the device code; it uses no scratch memory (private_segment_fixed_size 0); its static LDS fits one compute unit (at most
163,840 bytes); its LDS is addressed through address-space pointers and its global pointers are kernel arguments, so there is
no flat_* instruction (the fallback runs K2's decoder, which relies on global_* operations of one wavefront completing in issue
order); at most 128 VGPRs, which is what 16 wavefronts per CU need; and every kernel the library had before is, instruction
for instruction, what tools/kernel_asm_diff.py finds in the parent commit's device code."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import __graft_entry__ as entry

HIP = os.path.join("pim-compression_amd", "csrc", "snappy_hip.hip")
HEADER = "pim-compression_amd/csrc/snappy_k2_wide.hpp"


def _compile(src, out):
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(out)])


def _field(body, name):
    return int(re.search(r"^\s*\.amdhsa_" + name + r" (\d+)", body, re.M).group(1))


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("wide_codegen") / "device.s"
    _compile(os.path.join(ROOT, HIP), out)
    return out


def test_wide_kernel_is_present_within_one_cu_and_without_scratch_or_flat(device_asm):
    text = device_asm.read_text()
    m = re.search(r"^(_ZN10snappy_hip\d+k2_wide_kernelE\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, "k2_wide_kernel not found in the device code"
    body = m.group(2)
    assert _field(body, "private_segment_fixed_size") == 0
    assert _field(body, "group_segment_fixed_size") <= 163840
    assert re.findall(r"^\s*flat_\w+", body, re.M) == []
    assert _field(body, "next_free_vgpr") <= 128
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    mine = sorted(k for k in kernels if "k2_wide" in k)
    # (tests/test_abi_symbols.py counts K2's and K1's kernels by these two name parts)
    assert len(mine) == 1 and "decompress_blocks_kernel" not in mine[0] and "_blocks_" not in mine[0], mine


def test_kernels_of_the_parent_commit_are_unchanged(device_asm, tmp_path):
    """The parent commit's tree is taken from git (the parent of the commit that added snappy_k2_wide.hpp), compiled the same way
    and compared kernel by kernel.  A later change that alters one of those kernels on purpose retires this test."""
    git = ["git", "-C", ROOT]
    if subprocess.run(git + ["rev-parse", "--git-dir"], capture_output=True).returncode != 0:
        pytest.skip("not a git checkout: there is no parent commit to compare with")
    added = subprocess.run(git + ["log", "--diff-filter=A", "--format=%H", "--", HEADER], capture_output=True, text=True, check=True).stdout.split()
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
    assert sum(ln.startswith("SAME") for ln in lines) >= 26 and sum(ln.startswith("NEW") for ln in lines) == 1
