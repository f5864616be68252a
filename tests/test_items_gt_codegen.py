"""CPU test of the generated code of the raw / .sz compress calls with a table workspace
(pim-compression_amd/csrc/snappy_hip_items_gt.hip, the library's sixth source): exactly the four instances of
item_fragments_global_table_kernel, and no other kernel, are in that source's device code; none spills, uses scratch memory or
has a flat_* instruction (K1's table stores rely on the issue order of global_* stores: tests/test_abi_symbols.py); and each
instance takes no more vector registers and no more LDS than the container's compress_blocks_global_table_kernel of the same
form and table kind, read from a compile of snappy_hip.hip here: the limit is the product kernel's occupancy, whatever it is.

The trip ends in a convergent operation, as the persistent kernels of tests/test_check_codegen.py do: the kernel has
raw_compress_fragments_kernel's __syncthreads() behind the parse (a 64-thread workgroup: the compiler emits it as a wave
barrier), on top of the wave barrier finish_block() ends every block with."""
import os
import re
import subprocess

from conftest import ROOT

import __graft_entry__ as entry

CSRC = os.path.join(ROOT, "pim-compression_amd", "csrc")
INSTANCES = ((3, 512), (2, 512), (3, 0), (2, 0))


def _compile(src, out):
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(out)])


def _field(body, name):
    return int(re.search(r"^\s*\.amdhsa_" + name + r" (\d+)", body, re.M).group(1))


def _body(text, mangled_start):
    m = re.search(r"^(_ZN10snappy_hip\d+" + mangled_start + r"\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, mangled_start
    return m.group(2)


def test_the_sixth_source_holds_four_instances_within_the_product_kernels_occupancy(tmp_path):
    out, product_out = tmp_path / "items_gt.s", tmp_path / "product.s"
    _compile(os.path.join(CSRC, "snappy_hip_items_gt.hip"), out)
    _compile(os.path.join(CSRC, "snappy_hip.hip"), product_out)
    text, product = out.read_text(), product_out.read_text()
    kernels = sorted(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    want = sorted("_ZN10snappy_hip34item_fragments_global_table_kernelILi%dELj%dEEE" % inst for inst in INSTANCES)
    assert len(kernels) == 4 and [k[:len(w)] for k, w in zip(kernels, want)] == want, kernels        # no kernel of another header
    for name in kernels:                                                  # the existing codegen tests count kernels by these name parts
        assert not any(part in name for part in ("_blocks_", "check_", "raw_split_", "resize_", "k2_wide", "raw_vsplit")), name
    for form, cache in INSTANCES:
        body = _body(text, "item_fragments_global_table_kernelILi%dELj%dEEE" % (form, cache))
        assert _field(body, "private_segment_fixed_size") == 0, (form, cache)
        assert re.findall(r"^\s*flat_\w+", body, re.M) == [], (form, cache)
        assert re.findall(r"^\s*scratch_\w+", body, re.M) == [], (form, cache)
        assert len(re.findall(r"^\s*global_(?:load|store|atomic)", body, re.M)) >= 2, (form, cache)
        assert "; wave barrier" in body, (form, cache)
        assert re.findall(r"^\s*global_atomic_add", body, re.M), "d_result[2] is counted with an atomic add"
        base = _body(product, "compress_blocks_global_table_kernelILj64ELi%dELi1ELj%dEEE" % (form, cache))
        print("form %d cache %d: vgprs %d (product %d), LDS %d (product %d)" % (
            form, cache, _field(body, "next_free_vgpr"), _field(base, "next_free_vgpr"), _field(body, "group_segment_fixed_size"),
            _field(base, "group_segment_fixed_size")))
        assert _field(body, "next_free_vgpr") <= _field(base, "next_free_vgpr"), (form, cache)
        assert 0 < _field(body, "group_segment_fixed_size") <= _field(base, "group_segment_fixed_size"), (form, cache)
