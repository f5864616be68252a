"""CPU test of the generated code of the .sz source (pim-compression_amd/csrc/snappy_hip_sz.hip): its kernels are in the device
code and no others; none spills or uses scratch memory; their pointers, which come from items in memory (load_global_ptr), give
global_* instructions, never flat_* ones -- sz_decode_chunks_kernel runs K2's decoder, which relies on global_* operations of
one wavefront completing in issue order, and reads back what it wrote behind the same wait; the decode kernel keeps K2's eight
wavefronts per SIMD; the persistent ones keep their wavefront together from one draw to the next.  And every kernel of the two
sources the library had before is, instruction for instruction, what tools/kernel_asm_diff.py finds in the parent commit."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import __graft_entry__ as entry

KERNELS = ("crc32c_batch_kernel", "sz_index_kernel", "sz_plan_kernel", "sz_decode_chunks_kernel", "sz_finish_kernel", "sz_compress_plan_kernel",
           "sz_compress_chunks_kernel", "sz_chunk_crc_kernel", "sz_sizes_kernel", "sz_gather_kernel")
INSTANCES = {"sz_index_kernel": 2, "sz_compress_chunks_kernel": 2, "crc32c_batch_kernel": 2, "sz_decode_chunks_kernel": 2, "sz_chunk_crc_kernel": 2}   # <false / true>, K1's two forms, the two table forms
PERSISTENT = ("crc32c_batch_kernel", "sz_decode_chunks_kernel", "sz_chunk_crc_kernel")
NO_LDS = ("sz_index_kernel", "sz_finish_kernel", "sz_sizes_kernel", "sz_gather_kernel")
WIDE = ("sz_plan_kernel", "sz_compress_plan_kernel", "sz_compress_chunks_kernel")      # 1024-thread planners; K1's parse (as the raw fragment kernel)
CSRC = os.path.join("pim-compression_amd", "csrc")
OLD_HIPS = (os.path.join(CSRC, "snappy_hip.hip"), os.path.join(CSRC, "snappy_hip_raw_check_split.hip"))
NEW_HIP = os.path.join(CSRC, "snappy_hip_sz.hip")


def _compile(src, out):
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(out)])


def _field(body, name):
    return int(re.search(r"^\s*\.amdhsa_" + name + r" (\d+)", body, re.M).group(1))


def test_the_sz_kernels_cross_compile_without_scratch(tmp_path):
    out = tmp_path / "device.s"
    _compile(os.path.join(ROOT, NEW_HIP), out)
    text = out.read_text()
    for name in KERNELS:
        found = list(re.finditer(r"^(_ZN10snappy_hip\d+" + name + r"I?\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M))
        assert len(found) == INSTANCES.get(name, 1), (name, [m.group(1) for m in found])
        for m in found:
            body = m.group(2)
            assert _field(body, "private_segment_fixed_size") == 0, name
            assert re.findall(r"^\s*flat_\w+", body, re.M) == [], name
            assert re.findall(r"^\s*scratch_\w+", body, re.M) == [], name
            assert len(re.findall(r"^\s*global_(?:load|store|atomic)", body, re.M)) >= 3, name
            assert _field(body, "next_free_vgpr") <= 64 or name in WIDE, name                # eight wavefronts per SIMD, as K2
            if name in PERSISTENT:
                assert "; wave barrier" in body, name        # (see tests/test_check_codegen.py: the trip ends in a convergent operation)
            if name in NO_LDS:
                assert _field(body, "group_segment_fixed_size") == 0, name
    kernels = sorted(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    assert len(kernels) == sum(INSTANCES.get(k, 1) for k in KERNELS) and all(any(name in k for name in KERNELS) for k in kernels), kernels
    # the name parts the other sources' tests count their kernels by
    for part in ("check_", "raw_split_", "resize_", "k2_wide", "_blocks_", "raw_vsplit"):
        assert not any(part in k for k in kernels), part
    # the decode kernel's LDS: K2's stage and the CRC tables, nothing else
    lds = sorted(_field(m.group(2), "group_segment_fixed_size")
                 for m in re.finditer(r"^(_ZN10snappy_hip\d+sz_decode_chunks_kernel\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M))
    assert lds == [1536 + 1024, 1536 + 4096]


def test_kernels_of_the_other_sources_are_what_the_parent_commit_has(tmp_path):
    """The parent commit's tree is taken from git (the parent of the commit that added snappy_sz.hpp; HEAD while it is not
    committed), compiled the same way and compared kernel by kernel: all SAME, none NEW, none DIFF, none GONE."""
    git = ["git", "-C", ROOT]
    if subprocess.run(git + ["rev-parse", "--git-dir"], capture_output=True).returncode != 0:
        pytest.skip("not a git checkout: there is no parent commit to compare with")
    added = subprocess.run(git + ["log", "--diff-filter=A", "--format=%H", "--", CSRC + "/snappy_sz.hpp"], capture_output=True, text=True,
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
    assert same >= 45
