"""CPU tests of K1's parse in the four kernels that carry it besides the two product kernels (csrc/snappy_kernels.hpp:
LDS_TABLE_WAVE_COMPRESS in recompress_dirty_kernel, resize_recompress_kernel, raw_compress_fragments_kernel and
sz_compress_chunks_kernel): the unmodified kernel source under the wave emulator on the inputs that were built to reach the
edges of the strided scan batch and of the duplicate analysis' aliases (tests/k1_carrier_cases.py), in both forms of the
parse.  Every stream is the oracle's byte for byte, with the guard bytes and pages of the carriers' own emulated tests; and
every carrier's emulator statistics equal those of the product's LDS-table kernel on the same blocks, so that a carrier which
takes another path through the parse shows even where the bytes agree.

Each carrier and form runs in one child process (a write outside a guarded window is a fault there, not here) that prints
one record per call: what failed, if anything, and the statistics of the carrier's own library around that call -- the
carrier's emulator source built with a reader for the alias statistics (tests/emu_k1_carriers_lib.py), which the carrier's
binding and helpers then run."""
import functools
import json
import os
import subprocess
import sys

import pytest

import emu_k1_carriers_lib as ecl
import k1_carrier_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))
CARRIERS = ("raw", "sz", "update", "resize")
# the passes of a carrier whose blocks are the input's blocks, all of them parsed: their statistics are the product kernel's
PASSES = {"raw": ("",), "sz": ("",), "update": ("#a", "#b"), "resize": ("#a",)}
BATCHES, BY_HIT, BY_SHARED, BY_LIMIT, FULL = 11, 12, 13, 14, 15       # g_stream_stats (snappy_kernels.hpp)
ENTERED, CLEARED, KEPT, FALLBACK = 0, 1, 2, 3                         # g_alias_stats


# ---- in the child ----
def step(*what):
    print("step", *what, flush=True)


def _read(fn):
    import ctypes
    out = (ctypes.c_ulonglong * 16)()
    fn(out)
    return [int(x) for x in out]


def _record(L, key, inputs, body):
    """body() between two reads of the statistics of library L (a read clears them); an assertion that fails is the record's
    error and the run goes on, so that one report names every comparison a wrong parse breaks"""
    _read(L.emu_stream_stats), _read(L.emu_alias_stats)
    step(key)
    error = None
    try:
        body()
    except AssertionError as e:
        error = ("%s: %r" % (type(e).__name__, e))[:400]
    print("record " + json.dumps({"key": key, "inputs": inputs, "error": error, "stream": _read(L.emu_stream_stats), "alias": _read(L.emu_alias_stats)}),
          flush=True)


def _batch_body(calls, L, compress, check):
    """raw and .sz: every call of `calls` as it stands -- several items drawn by three wavefronts -- and, where it has more than
    one item, every item again as a call of its own, for the statistics of that input"""
    for call in calls:
        for one in [call] + ([call.alone(k) for k in range(len(call.items))] if len(call.items) > 1 else []):
            def body(c=one):
                r, b = compress(c)
                assert r == 0, "a kernel wrote in front of a window"
                for i, (plain, cap) in enumerate(c.items):
                    check(b, i, plain, c.block_size, cap, c.wants[i])
                assert [int(x) for x in b.result] == [c.max_units, len(c.items)], [int(x) for x in b.result]
                assert int(b.status[len(c.items)]) == 0x55 and int(b.out_len[len(c.items)]) == 0x5A5A5A5A5A5A5A5A   # nothing behind the arrays' last entry
            key = one.names[0] if len(one.items) == 1 else "group/%d" % one.block_size
            _record(L, key, one.names, body)


def body_raw(form):
    import emu_raw_lib as er
    import test_raw_emulated as t

    def check(b, i, plain, bs, cap, want):
        assert t.want_raw(plain, bs) == want
        assert t.check_compressed(b, i, plain, bs, cap)                 # status, length, bytes, the window's rest untouched

    _batch_body(kc.raw_calls(), ecl.lib("raw"), lambda c: er.compress(c.items, c.block_size, c.max_units, grid=3, form=form), check)


def body_sz(form):
    import emu_sz_lib as es
    import sz_cases as sz
    import test_sz_emulated as t

    def check(b, i, plain, chunk_len, cap, want):
        assert t.check_compressed(b, i, plain, chunk_len, cap) == want
        assert int(b.status[i]) == sz.OK

    _batch_body(kc.sz_calls(), ecl.lib("sz"), lambda c: es.compress(c.items, c.block_size, c.max_units, grid=3, form=form), check)


def body_update(form):
    import test_update_emulated as t
    L = ecl.lib("update")
    for name, data, bs in kc.inputs():
        for tag, c, writes, want in kc.update_calls(data, bs):
            def body():
                kc.expected_update(c, writes, want)
                r = t.check_ok(c, writes, form=form)                    # statuses, dirty count, bytes, offsets, guard bytes
                assert r.out[t.PAD:t.PAD + r.new_len].tobytes() == want
            _record(L, name + "#" + tag, [name], body)


def body_resize(form):
    import test_resize_emulated as t
    L = ecl.lib("resize")
    for name, data, bs in kc.inputs():
        for tag, c, keep_len, segments, want, parsed in kc.resize_calls(data, bs):
            def body():
                kc.expected_resize(c, keep_len, segments, want, parsed)
                assert t.check_ok(c, keep_len, segments, want=want, form=form).stream == want
            _record(L, name + "#" + tag, [name], body)


BODIES = {"raw": body_raw, "sz": body_sz, "update": body_update, "resize": body_resize}


# ---- in the parent ----
@functools.lru_cache(maxsize=None)
def _run(carrier, form):
    """{key: record} of one carrier in one form"""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import conftest, test_k1_carriers_emulated as t\n"
            "t.BODIES[sys.argv[2]](int(sys.argv[3]))\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code, HERE, carrier, str(form)], capture_output=True, text=True, timeout=1500)
    lines = out.stdout.strip().splitlines()
    last = next((ln for ln in reversed(lines) if ln.startswith("step ")), "none")
    assert out.returncode == 0 and lines and lines[-1] == "ok", \
        ("status %d (negative: a signal, i.e. an access outside a guarded buffer) at %s" % (out.returncode, last), out.stderr[-2000:])
    records = [json.loads(ln[7:]) for ln in lines if ln.startswith("record ")]
    res = {r["key"]: r for r in records}
    assert len(res) == len(records)
    return res


@functools.lru_cache(maxsize=None)
def _product(form):
    """{input: the 16 stream statistics of the product's LDS-table kernel in this form}, its stream being the oracle's"""
    import ctypes

    import emu_lib as emu
    import oracle_lib as oracle
    res = {}
    for name, data, bs in kc.inputs():
        out = (ctypes.c_ulonglong * 16)()
        emu.lib().emu_stream_stats(out)
        assert emu.compress(data, bs, kc.PRODUCT_VARIANT[form]) == oracle.compress(data, bs), name
        emu.lib().emu_stream_stats(out)
        res[name] = [int(x) for x in out]
    return res


@functools.lru_cache(maxsize=None)
def _product_alias():
    """{alias input: the 16 alias statistics of the product's LDS-table kernel in the stream form}"""
    import emu_k1_alias_lib as emu
    import oracle_lib as oracle
    res = {}
    for name, data, bs in kc.inputs():
        if kc.is_alias(name):
            emu.alias_stats()
            assert emu.compress(data, bs, kc.PRODUCT_VARIANT[3]) == oracle.compress(data, bs), name
            res[name] = list(emu.alias_stats())
    assert len(res) == 6
    return res


def _input_keys(carrier):
    """the records that hold one input's statistics, per pass"""
    return {p: [name + p for name, _, _ in kc.inputs()] for p in PASSES[carrier]}


def _sum(rows):
    return [sum(col) for col in zip(*rows)]


def _entries(got, want):
    """the statistics that differ: [(entry, the carrier's, the product kernel's)]"""
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]


def _report(differ):
    return "%d calls differ; (entry, carrier, product kernel):\n" % len(differ) + "\n".join("%s: %s" % kv for kv in list(differ.items())[:20])


def test_the_inputs_are_the_strided_and_the_alias_cases():
    import k1_alias_cases
    import k1_strided_cases
    names = [name for name, _, _ in kc.inputs()]
    assert len(names) == len(set(names)) == len(k1_strided_cases.cases()) + len(k1_alias_cases.cases()) == 77
    assert sum(kc.is_alias(n) for n in names) == 6 and sum(kc.is_built(n) for n in names) == 4
    assert sorted(i for _, idx in kc.groups() for i in idx) == list(range(77))


def test_sz_streams_of_the_alias_and_planted_inputs_show_the_parse():
    kc.assert_sz_inputs_stay_visible()


@pytest.mark.parametrize("form", kc.FORMS)
@pytest.mark.parametrize("carrier", CARRIERS)
def test_carrier_streams_are_the_oracles(carrier, form):
    """Every call of tests/k1_carrier_cases.py: statuses, lengths, counts, bytes and guards as the carrier's own emulated test
    checks them, the bytes being the oracle's."""
    res = _run(carrier, form)
    failed = {k: r["error"] for k, r in res.items() if r["error"]}
    assert not failed, failed
    calls = {"raw": len(kc.raw_calls()) + 77 - sum(len(c.items) == 1 for c in kc.raw_calls()),
             "sz": len(kc.sz_calls()) + 77 - sum(len(c.items) == 1 for c in kc.sz_calls()), "update": 2 * 77, "resize": 2 * 77}
    assert len(res) == calls[carrier]
    for keys in _input_keys(carrier).values():
        assert all(k in res for k in keys)


@pytest.mark.parametrize("form", kc.FORMS)
@pytest.mark.parametrize("carrier", CARRIERS)
def test_carrier_statistics_are_the_product_kernels(carrier, form):
    """The blocks a carrier parses are the input's blocks, so its 16 stream statistics are those of the product's LDS-table
    kernel in the same form (3501 / 2501), input by input -- and call by call where a call holds several inputs.  A
    difference means the carrier took another path.  (Resize (b) parses at most one block and is compared on bytes alone.)"""
    res, product = _run(carrier, form), _product(form)
    differ = {}
    for key, r in res.items():
        if carrier == "resize" and key.endswith("#b"):
            continue
        want = _sum([product[name] for name in r["inputs"]])
        if r["stream"] != want:
            differ[key] = _entries(r["stream"], want)
    assert not differ, _report(differ)


@pytest.mark.parametrize("carrier", CARRIERS)
def test_carrier_alias_statistics_are_the_product_kernels(carrier):
    """Stream form: the alias statistics of the six alias inputs against the product's LDS-table kernel."""
    res, product = _run(carrier, 3), _product_alias()
    differ = {}
    for p in PASSES[carrier]:
        for name, want in product.items():
            if res[name + p]["alias"] != want:
                differ[name + p] = _entries(res[name + p]["alias"], want)
    assert not differ, _report(differ)


@pytest.mark.parametrize("form", kc.FORMS)
@pytest.mark.parametrize("carrier", CARRIERS)
def test_carrier_reached_every_ending(carrier, form):
    """The conditions under which the comparisons above mean something, on the carrier's own counters and with the thresholds
    of tests/test_k1_strided_emulated.py and tests/test_k1_alias_emulated.py: the scan batch ran and ended in each of its four
    ways; in the stream form the constructed windows were taken, aliased lanes were found, and the loop over them ended in
    both of its ways without a window falling back."""
    res = _run(carrier, form)
    for p, keys in _input_keys(carrier).items():
        total = _sum([res[k]["stream"] for k in keys])
        taken, endings = total[BATCHES], total[BY_HIT:FULL + 1]
        print("%s%s form %d: batches %d, by hit / shared slot / limit / full %s" % (carrier, p, form, taken, endings))
        assert taken == sum(endings), (p, total)
        assert taken >= 200, (p, total)
        assert min(endings) >= 5, (p, total)
        if form == 3:
            for name, _, _ in kc.inputs():
                if kc.is_built(name):
                    assert res[name + p]["stream"][0] >= 20, (name + p, res[name + p]["stream"])      # windows taken by the stream form
            alias = _sum([res[name + p]["alias"] for name, _, _ in kc.inputs() if kc.is_alias(name)])
            print("%s%s: aliased lanes entered %d, cleared %d, kept %d, fallback windows %d" % (carrier, p, *alias[:4]))
            assert alias[ENTERED] == alias[CLEARED] + alias[KEPT], (p, alias)
            assert alias[CLEARED] >= 5 and alias[KEPT] >= 5, (p, alias)
            assert alias[FALLBACK] == 0, (p, alias)
