"""GPU tests (-m gpu) of K1's parse in the four kernels that carry it besides the two product kernels (update, resize, raw,
.sz): the calls of tests/k1_carrier_cases.py -- the inputs built to reach the edges of the strided scan batch and of the
duplicate analysis' aliases -- through the C ABI, as tests/test_k1_carriers_emulated.py sends them through the emulator, in
both forms of the parse.  Every stream is the oracle's byte for byte, with the guard bytes, statuses and lengths the carriers'
own GPU tests check, and is decoded again on the device."""
import numpy as np
import pytest

import k1_carrier_cases as kc
import raw_cases as rc
import sz_cases as sz
import test_gpu_raw as tr
import test_gpu_resize as tz
import test_gpu_sz as ts
import test_gpu_update as tu

pytestmark = pytest.mark.gpu
FORMS = pytest.mark.parametrize("form", kc.FORMS, ids=["stream", "bulk"])


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert binding.lib().snappy_hip_device_count() >= 1
    return binding


def _set_form(monkeypatch, form):
    """bit 0 of SNAPPY_HIP_K1_STREAM: the stream form of the LDS-table parse; the library reads it per call"""
    monkeypatch.setenv("SNAPPY_HIP_K1_STREAM", "1" if form == 3 else "0")


class Batch(tr.Batch):
    """test_gpu_raw.Batch with the source of input i behind kc.spare(i) bytes from a 16-byte boundary"""

    def __init__(self, call):
        import torch
        super().__init__(call.items)
        blob, at = bytearray(), []
        for i, plain in zip(call.indexes, call.plains):
            blob += bytes(-len(blob) % 16 + kc.spare(i))
            at.append(len(blob))
            blob += plain
        self.d_src = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()
        assert self.d_src.data_ptr() % 16 == 0
        self.src_at = np.array(at, dtype=np.int64)
        self.entries = [(self.d_src.data_ptr() + a, e[1], e[2], e[3]) for a, e in zip(at, self.entries)]
        self.alignments = {e[0] % 16 for e in self.entries}


@FORMS
def test_gpu_raw_compress_of_the_k1_inputs(shb, form, monkeypatch):
    _set_form(monkeypatch, form)
    alignments = set()
    for call in kc.raw_calls():
        bs, n = call.block_size, len(call.items)
        assert all(shb.raw_compress_bound(len(p), bs) == kc.raw_bound(len(p), bs) >= len(w) for p, w in zip(call.plains, call.wants))
        b = Batch(call)
        alignments |= b.alignments
        shb.raw_compress_batch(shb.make_raw_items(b.entries), n, bs, call.max_units, b.d_out_len, b.d_status, b.d_result)
        b.fetch()                                                       # the guard bytes between, in front of and behind the windows
        for i, name in enumerate(call.names):
            assert tr.check_compressed(b, i, call.wants[i], call.caps[i]), name      # status, length, bytes, the window's rest untouched
        assert b.result == [call.max_units, n], (bs, b.result)
        d = tr.gpu_decompress(shb, [(b.window(i)[:b.out_len[i]], len(p)) for i, p in enumerate(call.plains)])
        for i, p in enumerate(call.plains):
            assert (d.status[i], d.out_len[i]) == (rc.OK, len(p)) and d.window(i) == p, call.names[i]
    assert alignments == set(range(16))


@FORMS
def test_gpu_sz_compress_of_the_k1_inputs(shb, form, monkeypatch):
    kc.assert_sz_inputs_stay_visible()
    _set_form(monkeypatch, form)
    alignments = set()
    for call in kc.sz_calls():
        bs, n = call.block_size, len(call.items)
        assert all(shb.sz_compress_bound(len(p), bs) == kc.sz_bound(len(p), bs) >= len(w) for p, w in zip(call.plains, call.wants))
        b = Batch(call)
        alignments |= b.alignments
        shb.sz_compress_batch(shb.make_raw_items(b.entries), n, bs, call.max_units, b.d_out_len, b.d_status, b.d_result)
        b.fetch()
        for i, (name, want, cap) in enumerate(zip(call.names, call.wants, call.caps)):
            assert (b.status[i], b.out_len[i]) == (sz.OK, len(want)), (name, b.status[i], b.out_len[i], len(want))
            assert b.window(i) == want + ts.FILL * (cap - len(want)), name
        assert b.result == [call.max_units, n], (bs, b.result)
        d = ts.gpu_decompress(shb, [(b.window(i)[:b.out_len[i]], len(p)) for i, p in enumerate(call.plains)], call.max_units)      # CRCs compared
        for i, p in enumerate(call.plains):
            assert (d.status[i], d.out_len[i], d.bad[i]) == (sz.OK, len(p), sz.NONE) and d.window(i) == p, call.names[i]
        assert d.result == [call.max_units, n]
    assert alignments == set(range(16))


def _decodes_to(shb, stream, plain):
    import torch
    st, d_back = shb.decompress_resident(torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda())
    return st == 0 and bytes(d_back[:len(plain)].cpu().numpy()) == plain


@FORMS
def test_gpu_update_of_the_k1_inputs(shb, form, monkeypatch):
    _set_form(monkeypatch, form)
    for name, data, bs in kc.inputs():
        for tag, c, writes, want in kc.update_calls(data, bs):
            kc.expected_update(c, writes, want)
            r = tu.check_ok(shb, c, writes)                             # statuses, dirty count, length, bytes, offsets, guard bytes
            stream = r.out[tu.PAD:tu.PAD + r.new_len].tobytes()
            assert stream == want, (name, tag)
            assert _decodes_to(shb, stream, data), (name, tag)


@FORMS
def test_gpu_resize_of_the_k1_inputs(shb, form, monkeypatch):
    _set_form(monkeypatch, form)
    for name, data, bs in kc.inputs():
        for tag, c, keep_len, segments, want, parsed in kc.resize_calls(data, bs):
            kc.expected_resize(c, keep_len, segments, want, parsed)
            r = tz.check_ok(shb, c, keep_len, segments, want=want)      # statuses, parsed count, length, bytes, offsets, guard bytes
            assert r.stream == want, (name, tag)
            assert _decodes_to(shb, r.stream, data), (name, tag)
