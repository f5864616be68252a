"""GPU (-m gpu): the HIP kernels against the REFERENCE's recorded results (tests/golden/reference_digests.json, written by
tools/record_reference.py from the reference's own host codec) -- the oracle is not consulted, no reference checkout is
read.  tests/test_reference_differential.py holds the oracle and the wave emulator to the same records on the CPU."""
import hashlib

import numpy as np
import pytest

import datagen
import ref_lib
import reference_cases as rc
from conftest import golden_bytes

pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return binding


def to_dev(data):
    import torch
    t = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    if len(data):
        t[:len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return t


def gpu_compress(shb, data, bs):
    return bytes(shb.compress_resident(to_dev(data), bs, n=len(data)).cpu().numpy())


def gpu_decompress(shb, stream):
    st, out = shb.decompress_resident(to_dev(stream), stream_len=len(stream))
    return st, bytes(out.cpu().numpy())


# the default launch (both K1 kernels side by side), the LDS-table kernel alone, the global-table kernel alone
@pytest.mark.parametrize("env", [{}, {"SNAPPY_HIP_COMPRESS_VARIANT": "1"}, {"SNAPPY_HIP_LDS_WAVES": "0"}],
                         ids=["default", "lds-table-alone", "global-table-alone"])
def test_gpu_compress_equals_every_reference_record(shb, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    comp, _, _ = rc.load_fixture()
    assert len(comp) >= 900
    wrong = []
    for (cid, bs), rec in comp.items():
        data = rc.input_for(cid)
        assert len(data) == rec["n"], cid
        got = gpu_compress(shb, data, bs)
        if len(got) != rec["stream_len"] or sha(got) != rec["sha256"]:
            wrong.append((cid, bs, len(got), rec["stream_len"]))
    assert not wrong, (env, len(wrong), wrong[:10])


def test_drop_in_compress_equals_the_reference_records_above_one_mebibyte(shb):
    comp, _, _ = rc.load_fixture()
    big = [(k, r) for k, r in comp.items() if r["n"] > (1 << 20)]
    assert big
    for (cid, bs), rec in big:
        st, stream, _ = shb.compress_host(rc.input_for(cid), bs)
        assert st == 0 and len(stream) == rec["stream_len"] and sha(stream) == rec["sha256"], (cid, bs)


def test_gpu_decode_against_every_reference_record(shb):
    """Undamaged streams: status 0 and the reference's plaintext digest.  Damaged ones: K2 may be stricter than the
    reference, never laxer -- if K2 accepts, the reference accepted, with the same bytes."""
    _, dec, _ = rc.load_fixture()
    accepted_damaged = 0
    for cid, rec in dec.items():
        stream, _ = rc.stream_for(cid)
        st, out = gpu_decompress(shb, stream)
        if not rc.is_damaged(cid):
            assert rec["status"] == 0
            assert st == 0 and sha(out) == rec["sha256"], cid
            continue
        assert st in (0, 1), cid
        if st == 0:
            assert rec["status"] == 0 and sha(out) == rec["sha256"], cid
            accepted_damaged += 1
    assert accepted_damaged > 0              # damage inside a literal's payload leaves a valid stream: not everything is rejected


@pytest.mark.skipif(not ref_lib.available(), reason="oracle/_ref/dpu_snappy_ref did not travel with the tree (`%s`)" % ref_lib.MAKE_TARGET)
def test_reference_binary_decodes_gpu_streams(shb):
    """50 seeded cases: what the GPU compressed, the reference's own decoder turns back into the input."""
    r = np.random.default_rng(5150)
    text = golden_bytes("plrabn12.txt")
    for seed in range(50):
        n = int(r.integers(1, 200_000))
        bs = int(r.choice([31, 64, 700, 4096, 4097, 16384, 32768, 32769, 65535]))
        data = (datagen.lz_structured(n, seed), datagen.records(n, seed), datagen.text_random_interleave(text, n, seed),
                datagen.low_entropy(n, 4, seed))[seed % 4]
        stream = gpu_compress(shb, data, bs)
        st, back = ref_lib.decompress(stream)
        assert st == 0 and back == data, (seed, n, bs)
