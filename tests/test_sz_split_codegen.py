"""CPU test of the generated code of the split walk of .sz streams (pim-compression_amd/csrc/snappy_hip_sz_split.hip, the
library's fourth source): its five kernels, and no other, are in that source's device code; none spills or uses scratch memory;
their pointers, which come from items in memory (load_global_ptr), give global_* instructions, never flat_* ones; all but the
1024-thread plan fit eight wavefronts per SIMD; the anchor scan, the walkers, the join and the record use no LDS.  And every
kernel of the three sources the library had before is, instruction for instruction, what tools/kernel_asm_diff.py finds in the
parent commit."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import __graft_entry__ as entry

KERNELS = ("sz_split_plan_kernel", "sz_split_anchor_kernel", "sz_split_walk_kernel", "sz_split_join_kernel", "sz_split_record_kernel")
WIDE = ("sz_split_plan_kernel",)                # the 1024-thread planner
NO_LDS = KERNELS[1:]
CSRC = os.path.join("pim-compression_amd", "csrc")
OLD_HIPS = (os.path.join(CSRC, "snappy_hip.hip"), os.path.join(CSRC, "snappy_hip_raw_check_split.hip"), os.path.join(CSRC, "snappy_hip_sz.hip"))
NEW_HIP = os.path.join(CSRC, "snappy_hip_sz_split.hip")


def _compile(src, out):
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(out)])


def _field(body, name):
    return int(re.search(r"^\s*\.amdhsa_" + name + r" (\d+)", body, re.M).group(1))


def test_the_split_walks_kernels_cross_compile_without_scratch_flat_or_lds(tmp_path):
    out = tmp_path / "device.s"
    _compile(os.path.join(ROOT, NEW_HIP), out)
    text = out.read_text()
    for name in KERNELS:
        m = re.search(r"^(_ZN10snappy_hip\d+" + name + r"E\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
        assert m, name
        body = m.group(2)
        assert _field(body, "private_segment_fixed_size") == 0, name
        assert re.findall(r"^\s*flat_\w+", body, re.M) == [], name
        assert re.findall(r"^\s*scratch_\w+", body, re.M) == [], name
        assert len(re.findall(r"^\s*global_(?:load|store|atomic)", body, re.M)) >= 3, name
        assert _field(body, "next_free_vgpr") <= 64 or name in WIDE, name                # eight wavefronts per SIMD, as K2
        if name in NO_LDS:
            assert _field(body, "group_segment_fixed_size") == 0, name
            assert re.findall(r"^\s*ds_(?:read|write|load|store)\w*", body, re.M) == [], name
    kernels = sorted(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    assert len(kernels) == len(KERNELS) and all(any(name in k for name in KERNELS) for k in kernels), kernels      # no kernel of another header
    # the name parts the other sources' tests count their kernels by
    for part in ("check_", "raw_split_", "resize_", "k2_wide", "_blocks_", "raw_vsplit", "sz_index", "sz_plan", "sz_decode", "sz_finish", "crc32c"):
        assert not any(part in k for k in kernels), part


def test_kernels_of_the_older_sources_are_what_the_parent_commit_has(tmp_path):
    """The parent commit's tree is taken from git (the parent of the commit that added snappy_sz_split.hpp; HEAD while it is not
    committed), compiled the same way and compared kernel by kernel: all SAME, none NEW, none DIFF, none GONE -- snappy_hip_sz.hip
    among them, whose header now wraps its kernels in a guard and whose host code shares two helpers."""
    git = ["git", "-C", ROOT]
    if subprocess.run(git + ["rev-parse", "--git-dir"], capture_output=True).returncode != 0:
        pytest.skip("not a git checkout: there is no parent commit to compare with")
    added = subprocess.run(git + ["log", "--diff-filter=A", "--format=%H", "--", CSRC + "/snappy_sz_split.hpp"], capture_output=True, text=True,
                           check=True).stdout.split()
    parent = (added[-1] + "^") if added else "HEAD"
    if subprocess.run(git + ["rev-parse", "--verify", "--quiet", parent + "^{commit}"], capture_output=True).returncode != 0:
        pytest.skip("the history does not reach the parent commit")
    tree = tmp_path / "parent"
    tree.mkdir()
    tar = subprocess.run(git + ["archive", parent, CSRC, "include"], capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", str(tree)], input=tar, check=True)
    same = 0
    for k, hip in enumerate(OLD_HIPS):
        before, after = tmp_path / ("before%d.s" % k), tmp_path / ("after%d.s" % k)
        _compile(str(tree / hip), before)
        _compile(os.path.join(ROOT, hip), after)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_asm_diff.py"), str(before), str(after)], capture_output=True, text=True)
        lines = [ln for ln in out.stdout.split("\n") if ln.strip()]
        assert out.returncode == 0 and not [ln for ln in lines if ln.startswith(("DIFF", "NEW", "GONE"))], (hip, [ln for ln in lines if not ln.startswith("SAME")])
        same += sum(ln.startswith("SAME") for ln in lines)
    assert same >= 60
