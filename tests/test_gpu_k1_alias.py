"""GPU tests (-m gpu) of the aliases of the stream form's duplicate analysis (csrc/snappy_k1_stream.hpp: stream_analyse): the
windows of tests/k1_alias_cases.py through the C ABI, once per kernel kind, every stream compared with the oracle's byte for
byte and decoded again by K2.  The inputs of one block size are one batched K1 launch."""
import functools

import numpy as np
import pytest

import k1_alias_cases as cases
import oracle_lib as oracle

pytestmark = pytest.mark.gpu

# the default launch, the LDS-table kernel alone (512-slot analysis), the global-table kernel alone (256-slot analysis): the
# knobs of tests/test_gpu_parity.py
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
def _references():
    """{name: the oracle's stream}, computed once"""
    return {name: oracle.compress(data, bs) for name, data, bs in cases.cases()}


def _to_dev(data):
    import torch
    t = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    t[:len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return t


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_aliased_windows_on_the_gpu_are_the_oracles(shb, shape, monkeypatch):
    import torch
    for k, v in SHAPES[shape].items():
        monkeypatch.setenv(k, v)
    refs = _references()
    for bs in cases.BLOCKS:
        group = [(name, data) for name, data, b in cases.cases() if b == bs]
        jobs = [(_to_dev(data), len(data), shb.CompressWorkspace(len(data), bs, scratch=(i == 0))) for i, (name, data) in enumerate(group)]
        shb.compress_blocks_batch(jobs)                                       # one K1 launch for the block size
        for (name, data), (d_in, n, ws) in zip(group, jobs):
            d_stream = torch.empty(ws.stream_capacity(n) + 16, dtype=torch.uint8, device="cuda")
            shb.compact(n, ws, d_stream)
            got = bytes(d_stream[:int(ws.stream_len.item())].cpu().numpy())
            assert got == refs[name], (shape, name)
            st, out = shb.decompress_resident(d_stream[:len(got)], stream_len=len(got))   # K2 on what K1 wrote
            assert st == 0 and bytes(out.cpu().numpy()) == data, (shape, name)
