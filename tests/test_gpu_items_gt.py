"""GPU tests (-m gpu) of the raw / .sz compress calls that take a table workspace (snappy_hip_raw_compress_batch_tables,
snappy_hip_sz_compress_batch_tables) through the C ABI.  Every test runs the new call and the base call on the same items --
sources GAP bytes apart, destinations between guard bytes -- and compares everything the contract names: every d_out_len[i],
every d_status[i], d_result[0] and [1], and every byte of the destination buffer, guard bytes included.  d_result[2] and [3]
are the new call's own; the word behind them keeps its sentinel.  Where expected bytes are stated they are the oracle's
(k1_carrier_cases' wants, convert(oracle.compress(...)), write_sz_oracle)."""
import hashlib

import numpy as np
import pytest

import k1_carrier_cases as kc
import raw_cases as rc
import sz_cases as sz
import test_gpu_k1_carriers as tk
import test_gpu_raw as tr
import test_gpu_sz as ts
from conftest import golden_bytes

pytestmark = pytest.mark.gpu
FMTS = pytest.mark.parametrize("fmt", ["raw", "sz"])
SENTINEL = 0x77
TABLE = 65536
ERR_ARG = 2


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert binding.lib().snappy_hip_device_count() >= 1
    return binding


@pytest.fixture(scope="module")
def mix(shb):
    """16 MiB of the Silesia-mix (text, xml, structured binary, noise), on the host"""
    import torch
    import silesia_mix
    st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(golden_bytes("xml.snappy"), dtype=np.uint8).copy()).cuda())
    xml = d_xml.cpu().numpy()
    assert st == 0 and hashlib.sha256(xml.tobytes()).hexdigest() == silesia_mix.XML_TXT_SHA256
    unit = silesia_mix.build_unit(xml, seed=0)
    assert unit.size >= 16 << 20
    return unit[:16 << 20].tobytes()


@pytest.fixture(scope="module")
def tables(shb):
    """the full workspace, never initialised by anyone but the tests that say so"""
    return shb.compress_tables()


def _five_words(b):
    import torch
    b.d_result = torch.full((5,), SENTINEL, dtype=torch.int32, device="cuda")
    return b


def _call(shb, fmt, new, b, bs, max_units, d_tables=None):
    items = shb.make_raw_items(b.entries)
    if new:
        (shb.raw_compress_batch_tables if fmt == "raw" else shb.sz_compress_batch_tables)(items, b.n, bs, max_units, b.d_out_len, b.d_status, b.d_result,
                                                                                         d_tables=d_tables)
    else:
        (shb.raw_compress_batch if fmt == "raw" else shb.sz_compress_batch)(items, b.n, bs, max_units, b.d_out_len, b.d_status, b.d_result)
    b.fetch()                                                           # the guard bytes between, in front of and behind the windows
    return b


def both(shb, fmt, make_batch, bs, max_units, d_tables):
    """the base call, then the new call, on batches make_batch() builds alike -> the new call's batch, held to the base call's"""
    base = _call(shb, fmt, False, _five_words(make_batch()), bs, max_units)
    b = _call(shb, fmt, True, _five_words(make_batch()), bs, max_units, d_tables)
    assert b.status == base.status and b.out_len == base.out_len
    assert b.result[:2] == base.result[:2] and base.result[2:] == [SENTINEL] * 3
    assert b.result[3:] == [0, SENTINEL], b.result
    assert (b.buf == base.buf).all(), int(np.argmax(b.buf != base.buf))
    return b


def units_of(plains, bs):
    return sum(-(-len(p) // bs) for p in plains)


def want_of(fmt, plain, bs):
    return tr.want_raw(plain, bs) if fmt == "raw" else sz.write_sz_oracle(plain, bs)


def round_trip(shb, fmt, b, plains, max_units):
    if fmt == "raw":
        d = tr.gpu_decompress(shb, [(b.window(i)[:b.out_len[i]], len(p)) for i, p in enumerate(plains)])
        for i, p in enumerate(plains):
            assert (d.status[i], d.out_len[i]) == (rc.OK, len(p)) and d.window(i) == p, i
    else:
        d = ts.gpu_decompress(shb, [(b.window(i)[:b.out_len[i]], len(p)) for i, p in enumerate(plains)], max_units)      # CRCs compared
        for i, p in enumerate(plains):
            assert (d.status[i], d.out_len[i], d.bad[i]) == (sz.OK, len(p), sz.NONE) and d.window(i) == p, i


# ---- K1's constructed inputs ----
@FMTS
def test_gpu_carrier_calls_through_global_table_wavefronts(shb, tables, fmt, monkeypatch):
    """every group call of k1_carrier_cases on three global-table wavefronts (SNAPPY_HIP_GT_WAVES=3: the groups are small):
    bytes equal the case's wants, sources at all sixteen alignments, d_result[2] = the fragments"""
    if fmt == "sz":
        kc.assert_sz_inputs_stay_visible()
    monkeypatch.setenv("SNAPPY_HIP_GT_WAVES", "3")
    alignments = set()
    for call in (kc.raw_calls() if fmt == "raw" else kc.sz_calls()):
        b = both(shb, fmt, lambda: tk.Batch(call), call.block_size, call.max_units, tables)
        alignments |= b.alignments
        for i, name in enumerate(call.names):
            assert tr.check_compressed(b, i, call.wants[i], call.caps[i]), name
        assert b.result[:3] == [call.max_units, len(call.items), call.max_units], (call.block_size, b.result)
    assert alignments == set(range(16))


@FMTS
def test_gpu_carrier_items_alone_take_the_small_batch_rule(shb, tables, fmt):
    """every input as a call of its own, no knob set: a handful of fragments is the LDS form's, d_result[2] = 0, same bytes"""
    for call in (kc.raw_calls() if fmt == "raw" else kc.sz_calls()):
        for k in range(len(call.items)):
            one = call.alone(k)
            b = both(shb, fmt, lambda: tk.Batch(one), one.block_size, one.max_units, tables)
            assert tr.check_compressed(b, 0, one.wants[0], one.caps[0]), one.names[0]
            assert b.result[:3] == [one.max_units, 1, 0], (one.names[0], b.result)


# ---- many fragments per wavefront ----
def carve(mix, sizes, at=0):
    """items of these sizes cut from the mix one behind the other"""
    out = []
    for n in sizes:
        out.append(mix[at:at + n])
        at += n
    assert at <= len(mix)
    return out


@FMTS
def test_gpu_many_fragments_per_wavefront_default_grid(shb, tables, mix, fmt):
    """block size 256 and at least three fragments per wavefront slot of the device (6 MiB on a whole MI355X): every wavefront
    of the default grid takes fragment after fragment, of item after item"""
    import torch
    props = torch.cuda.get_device_properties(0)
    slots = props.multi_processor_count * (props.max_threads_per_multi_processor // 64)
    bs = 256
    total = 3 * slots * bs + 12345
    assert total <= len(mix)
    sizes = [total // 2, 1, 0, 70001, 255, 256, 257]
    sizes.append(total - sum(sizes))
    plains = carve(mix, sizes)
    units = units_of(plains, bs)
    assert units >= 3 * slots
    bound = shb.raw_compress_bound if fmt == "raw" else shb.sz_compress_bound
    items = [(p, bound(len(p), bs)) for p in plains]
    b = both(shb, fmt, lambda: tr.Batch(items), bs, units, tables)
    assert b.status[:len(plains)] == [rc.OK] * len(plains) and b.result[:3] == [units, len(plains), units]
    for i in (1, 2, 3, 4, 5, 6):                                            # (the small items against the oracle; the large ones decode below)
        assert b.window(i)[:b.out_len[i]] == want_of(fmt, plains[i], bs), i
    round_trip(shb, fmt, b, plains, units)


@FMTS
def test_gpu_many_fragments_per_wavefront_capped_grid(shb, tables, mix, fmt, monkeypatch):
    """512 fragments of 32 KiB on 64 wavefronts (SNAPPY_HIP_GT_WAVES, read per call): about eight each"""
    monkeypatch.setenv("SNAPPY_HIP_GT_WAVES", "64")
    bs = 32768
    plains = carve(mix, [100 * bs, 200 * bs + 1, 3 * bs - 1, 208 * bs])
    units = units_of(plains, bs)
    assert units == 512
    bound = shb.raw_compress_bound if fmt == "raw" else shb.sz_compress_bound
    items = [(p, bound(len(p), bs)) for p in plains]
    b = both(shb, fmt, lambda: tr.Batch(items), bs, units, tables)
    assert b.status[:4] == [rc.OK] * 4 and b.result[:3] == [512, 4, 512]
    assert b.window(2)[:b.out_len[2]] == want_of(fmt, plains[2], bs)
    round_trip(shb, fmt, b, plains, units)


@FMTS
@pytest.mark.parametrize("bs", [4096, 8192, 8193, 32768])
def test_gpu_both_table_kinds_and_the_switch_between_them(shb, tables, mix, fmt, bs, monkeypatch):
    """the filter alone up to 8192, the slot cache from 8193: ~100 fragments on 16 wavefronts, bytes the oracle's"""
    monkeypatch.setenv("SNAPPY_HIP_GT_WAVES", "16")
    plains = carve(mix, [40 * bs + 7, 0, bs, 59 * bs - 1, 1], at=5 << 20)
    units = units_of(plains, bs)
    wants = [want_of(fmt, p, bs) for p in plains]
    items = [(p, len(w) + (i % 2) * 11) for i, (p, w) in enumerate(zip(plains, wants))]
    b = both(shb, fmt, lambda: tr.Batch(items), bs, units, tables)
    for i, w in enumerate(wants):
        assert tr.check_compressed(b, i, w, items[i][1]), i
    assert b.result[:3] == [units, len(plains), units]


@FMTS
def test_gpu_tables_never_initialised_and_the_smallest_workspace(shb, mix, fmt, monkeypatch):
    """tables of 0xff, then of random bytes, then the same call with room for exactly one table (one wavefront takes every
    fragment): identical outputs, the base call's"""
    import torch
    monkeypatch.setenv("SNAPPY_HIP_GT_WAVES", "32")
    bs = 32768
    plains = carve(mix, [33 * bs + 5, 2 * bs, 17], at=9 << 20)
    units = units_of(plains, bs)
    bound = shb.raw_compress_bound if fmt == "raw" else shb.sz_compress_bound
    items = [(p, bound(len(p), bs)) for p in plains]
    bufs = []
    for fill in ("ff", "random", "one table"):
        if fill == "ff":
            t = torch.full((256 + 32 * TABLE,), 0xff, dtype=torch.uint8, device="cuda")
        else:
            size = 256 + (32 if fill == "random" else 1) * TABLE
            t = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=size, dtype=np.uint8)).cuda()
        assert t.data_ptr() % 256 == 0
        b = both(shb, fmt, lambda: tr.Batch(items), bs, units, t)
        assert b.status[:3] == [rc.OK] * 3 and b.result[:3] == [units, 3, units], (fill, b.result)
        bufs.append(b.buf)
    assert (bufs[0] == bufs[1]).all() and (bufs[0] == bufs[2]).all()
    for bs2 in (4096,):                                                    # the filter-alone kind on one table, too
        items2 = [(p, bound(len(p), bs2)) for p in plains[1:]]
        b = both(shb, fmt, lambda: tr.Batch(items2), bs2, units_of(plains[1:], bs2), t)
        assert b.result[2] == units_of(plains[1:], bs2)


# ---- statuses, refusals, the small-batch rule ----
@FMTS
def test_gpu_statuses_are_the_base_calls(shb, tables, fmt, monkeypatch):
    monkeypatch.setenv("SNAPPY_HIP_GT_WAVES", "5")
    bs = 1000
    text = golden_bytes("plrabn12.txt")
    plains = [text[1000 * k:1000 * k + n] for k, n in enumerate((2500, 0, 999, 3001, 0, 1, 700))]        # 3 + 0 + 1 + 4 + 0 + 1 + 1 units
    wants = [want_of(fmt, p, bs) for p in plains]
    need = units_of(plains, bs)
    # DST_TOO_SMALL: the needed size reported, dst untouched; the others exact
    short = [(p, len(w) - 1 if i in (0, 3) else len(w)) for i, (p, w) in enumerate(zip(plains, wants))]
    b = both(shb, fmt, lambda: tr.Batch(short), bs, need, tables)
    assert [tr.check_compressed(b, i, w, short[i][1]) for i, w in enumerate(wants)] == [i not in (0, 3) for i in range(7)]
    assert b.result[:3] == [need, 5, need]
    # TOO_LARGE beyond max_fragments: the items in front of the cut complete
    items = [(p, len(w)) for p, w in zip(plains, wants)]
    for max_units in (need - 1, 7, 4, 3, 0):
        b = both(shb, fmt, lambda: tr.Batch(items), bs, max_units, tables)
        first = ok = done = 0
        for i, p in enumerate(plains):
            n = -(-len(p) // bs)
            if n and first + n > max_units:
                assert (b.status[i], b.out_len[i]) == (rc.TOO_LARGE, 0) and b.window(i) == tr.FILL * len(wants[i]), i
            else:
                ok += tr.check_compressed(b, i, wants[i], len(wants[i]))
            first += n
        assert b.result[:2] == [need, ok] and (b.result[2] > 0) == (max_units > 0)
    # a null src, a null src of no bytes, src_len of 4 GiB, a null dst, an empty item
    bad = [(b"abc", 64, 1), (b"", 16, 1, 0), (b"abc", 64, 0, 1 << 32), (b"abcd" * 10, 0, 2), (b"", 16), (plains[0], len(wants[0]))]
    b = both(shb, fmt, lambda: tr.Batch(bad), bs, 8, tables)
    assert b.status[:6] == [rc.INVALID, rc.OK, rc.TOO_LARGE, rc.DST_TOO_SMALL, rc.OK, rc.OK]
    assert b.window(4)[:b.out_len[4]] == want_of(fmt, b"", bs) and tr.check_compressed(b, 5, wants[0], len(wants[0]))
    # count == 0: accepted, all four words written
    b = both(shb, fmt, lambda: tr.Batch([]), bs, 4, tables)
    assert b.result == [0, 0, 0, 0, SENTINEL]


@FMTS
def test_gpu_refusals_enqueue_nothing(shb, tables, fmt):
    """a null, misaligned and one-byte-short d_tables, and the base call's own cases: SNAPPY_HIP_ERR_ARG, every output array keeps
    its sentinel"""
    import torch
    L = shb.lib()
    fn = L.snappy_hip_raw_compress_batch_tables if fmt == "raw" else L.snappy_hip_sz_compress_batch_tables
    bs = 1000
    plain = golden_bytes("plrabn12.txt")[:2500]
    b = _five_words(tr.Batch([(plain, 4000)]))
    items = shb.make_raw_items(b.entries)
    need = (shb.raw_compress_scratch_bytes if fmt == "raw" else shb.sz_compress_scratch_bytes)(bs, 1, 3)
    scratch = torch.full((need + 512,), 0xCD, dtype=torch.uint8, device="cuda")
    sp = (scratch.data_ptr() + 255) & ~255
    tp, tn = tables.data_ptr(), tables.numel()
    assert tp % 256 == 0 and tn >= 256 + TABLE
    good = [items.data_ptr(), 1, bs, 3, b.d_out_len.data_ptr(), b.d_status.data_ptr(), b.d_result.data_ptr(), sp, need, tp, tn, None]

    def changed(**kw):
        names = ["items", "count", "bs", "max_units", "out_len", "status", "result", "scratch", "scratch_bytes", "tables", "tables_bytes", "stream"]
        return [kw.get(n, v) for n, v in zip(names, good)]

    refused = [changed(tables=None), changed(tables=tp + 16), changed(tables=tp + 128), changed(tables_bytes=256 + TABLE - 1), changed(tables_bytes=0),
               changed(items=None), changed(out_len=None), changed(status=None), changed(result=None), changed(bs=0), changed(bs=65536),
               changed(scratch=None), changed(scratch=sp + 16), changed(scratch_bytes=need - 1)]
    for args in refused:
        assert fn(*args) == ERR_ARG, args
        assert shb.lib().snappy_hip_last_error()
    torch.cuda.synchronize()
    b.fetch()
    assert b.status == [0x55, 0x55] and b.out_len == [0x5A5A5A5A5A5A5A5A] * 2 and b.result == [SENTINEL] * 5
    assert (b.buf == rc.GUARD).all() and bool((scratch == 0xCD).all().item())
    assert fn(*changed(tables_bytes=256 + TABLE)) == 0                      # room for exactly one table is valid
    b.fetch()
    assert b.status[0] == rc.OK and b.window(0)[:b.out_len[0]] == want_of(fmt, plain, bs) and b.result[3:] == [0, SENTINEL]


@FMTS
def test_gpu_small_batch_rule(shb, tables, fmt):
    """four items of one fragment each: the base call's fragment kernel, d_result[2] = 0, the same bytes"""
    bs = 32768
    text = golden_bytes("plrabn12.txt")
    plains = [text[k * 30000:k * 30000 + 20000 + k] for k in range(4)]
    wants = [want_of(fmt, p, bs) for p in plains]
    items = [(p, len(w)) for p, w in zip(plains, wants)]
    b = both(shb, fmt, lambda: tr.Batch(items), bs, 4, tables)
    for i, w in enumerate(wants):
        assert tr.check_compressed(b, i, w, len(w)), i
    assert b.result == [4, 4, 0, 0, SENTINEL]
