"""CPU test of the generated code of the .sz index and range calls (pim-compression_amd/csrc/snappy_hip_sz_ranges.hip, the
library's fifth source): its five kernels, and no other, are in that source's device code; none spills, uses scratch memory or has
a flat_* instruction (their pointers come from descs, ranges and items in memory: load_global_ptr); the decode kernel fits eight
wavefronts per SIMD and takes no more LDS than sz_decode_chunks_kernel<1>, read from a compile of snappy_hip_sz.hip here.  And
every kernel of the four sources the library had before is, instruction for instruction, what tools/kernel_asm_diff.py finds in
the parent commit."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import __graft_entry__ as entry

KERNELS = ("sz_shadow_items_kernel", "sz_index_export_kernel", "sz_range_pieces_kernel", "sz_decompress_ranges_kernel", "sz_range_finish_kernel")
DECODE = "sz_decompress_ranges_kernel"
CSRC = os.path.join("pim-compression_amd", "csrc")
OLD_HIPS = (os.path.join(CSRC, "snappy_hip.hip"), os.path.join(CSRC, "snappy_hip_raw_check_split.hip"), os.path.join(CSRC, "snappy_hip_sz.hip"),
            os.path.join(CSRC, "snappy_hip_sz_split.hip"))
NEW_HIP = os.path.join(CSRC, "snappy_hip_sz_ranges.hip")
SPLIT_KERNELS = ("sz_split_plan_kernel", "sz_split_anchor_kernel", "sz_split_walk_kernel", "sz_split_join_kernel", "sz_split_record_kernel")


def _compile(src, out):
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(out)])


def _field(body, name):
    return int(re.search(r"^\s*\.amdhsa_" + name + r" (\d+)", body, re.M).group(1))


def _body(text, name):
    m = re.search(r"^(_ZN10snappy_hip\d+" + name + r"\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, name
    return m.group(2)


def test_the_fifth_sources_kernels_cross_compile_without_scratch_or_flat(tmp_path):
    out, sz_out = tmp_path / "device.s", tmp_path / "sz.s"
    _compile(os.path.join(ROOT, NEW_HIP), out)
    _compile(os.path.join(ROOT, CSRC, "snappy_hip_sz.hip"), sz_out)
    text = out.read_text()
    for name in KERNELS:
        body = _body(text, name)
        assert _field(body, "private_segment_fixed_size") == 0, name
        assert re.findall(r"^\s*flat_\w+", body, re.M) == [], name
        assert re.findall(r"^\s*scratch_\w+", body, re.M) == [], name
        assert len(re.findall(r"^\s*global_(?:load|store|atomic)", body, re.M)) >= 2, name
    kernels = sorted(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    assert len(kernels) == len(KERNELS) and all(any(name in k for name in KERNELS) for k in kernels), kernels      # no kernel of another header
    decode = _body(text, DECODE)
    assert _field(decode, "next_free_vgpr") <= 64                                        # eight wavefronts per SIMD, as K2
    base = _body(sz_out.read_text(), "sz_decode_chunks_kernelILi1E")
    assert 0 < _field(decode, "group_segment_fixed_size") <= _field(base, "group_segment_fixed_size")
    assert re.findall(r"^\s*global_atomic_u?min_(?:x2|u64)", decode, re.M), "the verdict is a 64-bit atomic minimum"


def test_kernels_of_the_older_sources_are_what_the_parent_commit_has(tmp_path):
    """The parent commit's tree is taken from git (the parent of the commit that added snappy_sz_ranges.hpp; HEAD while it is not
    committed), compiled the same way and compared kernel by kernel: all SAME, none NEW, none DIFF, none GONE -- and the fourth
    source holds exactly its five kernels, although its host code now shares the walk's launches."""
    git = ["git", "-C", ROOT]
    if subprocess.run(git + ["rev-parse", "--git-dir"], capture_output=True).returncode != 0:
        pytest.skip("not a git checkout: there is no parent commit to compare with")
    added = subprocess.run(git + ["log", "--diff-filter=A", "--format=%H", "--", CSRC + "/snappy_sz_ranges.hpp"], capture_output=True, text=True,
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
        if hip.endswith("snappy_hip_sz_split.hip"):
            kernels = sorted(re.findall(r"^\s*\.amdhsa_kernel (\S+)", after.read_text(), re.M))
            assert len(kernels) == 5 and all(any(name in k for name in SPLIT_KERNELS) for k in kernels), kernels
    assert same >= 65
