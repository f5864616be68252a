"""GPU tests (-m gpu) of K1's strided scan batch and its long literals (csrc/snappy_kernels.hpp: strided_scan_batch,
emit_literal): incompressible data, and data that moves into and out of it, through the C ABI in three launch shapes, every
stream compared with the oracle's byte for byte and decoded again by K2."""
import functools

import numpy as np
import pytest

import k1_strided_cases as cases
import oracle_lib as oracle

pytestmark = pytest.mark.gpu

# the default launch (both K1 kernels on one container where it is large enough), the LDS-table kernel alone, the
# global-table kernel alone (the knobs of tests/test_gpu_parity.py)
SHAPES = {"default": {}, "lds_table": {"SNAPPY_HIP_COMPRESS_VARIANT": "1"}, "global_table": {"SNAPPY_HIP_LDS_WAVES": "0"}}


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return binding


@functools.lru_cache(maxsize=None)
def _inputs():
    """{name: (data, block size)}: the emulated test's inputs, and all 64 blocks of the planted construction cut into blocks
    of 4096, 32768 and 65535 bytes"""
    out = {name: (data, bs) for name, data, bs in cases.cases() if name != "planted"}
    for bs in (4096, 32768, 65535):
        out["planted/%d" % bs] = (cases.planted(), bs)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name):
    data, bs = _inputs()[name]
    return oracle.compress(data, bs, threads=8)


def _to_dev(data):
    import torch
    t = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    t[:len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return t


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_strided_scan_on_the_gpu_is_the_oracles(shb, shape, monkeypatch):
    for k, v in SHAPES[shape].items():
        monkeypatch.setenv(k, v)
    for name, (data, bs) in _inputs().items():
        ref = _reference(name)
        d_stream = shb.compress_resident(_to_dev(data), bs, n=len(data))
        got = bytes(d_stream.cpu().numpy())
        assert got == ref, (shape, name)
        st, out = shb.decompress_resident(d_stream, stream_len=len(got))   # K2 on what K1 wrote
        assert st == 0 and bytes(out.cpu().numpy()) == data, (shape, name)
