"""CPU tests of the raw / .sz compress calls with K1's global-table wavefronts: the UNMODIFIED kernel of
pim-compression_amd/csrc/snappy_items_gt.hpp on the lockstep wave emulator, between the base calls' own planner, CRC, sizes and
gather kernels (tests/emu/emu_items_gt.cpp).  Every dst is a window of exactly its capacity between inaccessible pages and every
src ends at one, so a byte written outside a window or read behind a source is a fault -- a legitimate failure here, which is
why every body runs in a child process that names the step it is on.  The tables are junk, as a workspace nobody initialised.

Expected bytes come from the oracle only: raw_cases.trs.convert(oracle.compress(...)) and sz_cases.write_sz_oracle.  Statuses
of refused items are compared, word for word, with what the base calls' emulator libraries answer for the same items."""
import os
import subprocess
import sys

import pytest

import datagen
import emu_items_gt_lib as eg
import k1_carrier_cases as kc
import raw_cases as rc
import sz_cases as sz
from conftest import golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = bytes([rc.GUARD])
FORMATS = ("raw", "sz")
KINDS = (True, False)                  # the 512-slot cache in front of the table; the filter alone
SENTINEL_STATUS, SENTINEL_LEN = 0x55, 0x5A5A5A5A5A5A5A5A


def step(*what):
    print("step", *what, flush=True)


def want_of(fmt, plain, bs):
    import oracle_lib as oracle
    return rc.trs.convert(oracle.compress(plain, bs)) if fmt == "raw" else sz.write_sz_oracle(plain, bs)


def check_item(b, i, want, capacity):
    """status, length and every byte of the window of item i against the expected stream at this capacity"""
    w = b.window(i)
    if len(want) <= capacity:
        assert (int(b.status[i]), int(b.out_len[i])) == (rc.OK, len(want)), (i, int(b.status[i]), int(b.out_len[i]), len(want))
        assert w[:len(want)] == want, (i, next(k for k in range(len(want)) if w[k] != want[k]))
        assert w[len(want):] == FILL * (capacity - len(want)), i
    else:
        assert (int(b.status[i]), int(b.out_len[i])) == (rc.DST_TOO_SMALL, len(want)), (i, int(b.status[i]), int(b.out_len[i]), len(want))
        assert w == FILL * capacity, i
    return len(want) <= capacity


def nothing_behind(b):
    assert int(b.status[b.n]) == SENTINEL_STATUS and int(b.out_len[b.n]) == SENTINEL_LEN


# ---- K1's constructed inputs: the seventh carrier ----
def body_carriers(fmt, form, cached):
    calls = kc.raw_calls() if fmt == "raw" else kc.sz_calls()
    for call in calls:
        step(fmt, "group", call.block_size, "items", len(call.items))
        r, b = eg.compress(fmt, call.items, call.block_size, call.max_units, grid=3, form=form, cached=bool(cached),
                           spares=[kc.spare(i) for i in call.indexes])
        assert r == 0, "a kernel wrote in front of a window"
        for i, (plain, cap) in enumerate(call.items):
            assert len(call.wants[i]) <= cap
            assert check_item(b, i, call.wants[i], cap), call.names[i]
        assert [int(x) for x in b.result] == [call.max_units, len(call.items), call.max_units, 0], [int(x) for x in b.result]
        nothing_behind(b)


# ---- one wavefront, many fragments: a table left by a fragment of another item ----
def many_fragment_items():
    """(plaintexts, bytes in front of each source): text, random bytes, zeros, a 1-byte item, an empty item, the text again, and
    the text with its source off alignment"""
    text = golden_bytes("alice.txt")
    plains = [text, datagen.random_bytes(40000, seed=5), datagen.zeros(70000), b"q", b"", text, text]
    return plains, [0, 0, 0, 0, 0, 0, kc.spare(6)]


def body_one_wavefront(fmt, bs):
    plains, spares = many_fragment_items()
    assert 1 <= spares[6] <= 16
    wants = [want_of(fmt, p, bs) for p in plains]
    units = sum(-(-len(p) // bs) for p in plains)
    items = [(p, len(w) + (i % 2) * 5) for i, (p, w) in enumerate(zip(plains, wants))]
    for form in kc.FORMS:
        for cached in KINDS:
            if bs < 4096 and (form, cached) != (2, False):   # (block sizes 1 and 256, up to 110,000 fragments: the instance the call chooses there)
                continue
            tables = eg.junk_tables(1, seed=bs)
            windows = []
            for run in ("junk tables", "the tables the first run left"):
                step(fmt, bs, "form", form, "cached", cached, run)
                r, b = eg.compress(fmt, items, bs, units, grid=1, form=form, cached=cached, tables=tables, spares=spares)
                assert r == 0, "a kernel wrote in front of a window"
                for i, want in enumerate(wants):
                    assert check_item(b, i, want, items[i][1]), i
                assert [int(x) for x in b.result] == [units, len(items), units, 0], [int(x) for x in b.result]
                nothing_behind(b)
                windows.append([b.window(i) for i in range(len(items))])
            assert windows[0] == windows[1]


# ---- statuses: the base emulator calls' answers, word for word ----
def base_compress(fmt, items, bs, max_units, grid):
    if fmt == "raw":
        import emu_raw_lib as er
        return er.compress(items, bs, max_units, grid=grid)
    import emu_sz_lib as es
    return es.compress(items, bs, max_units, grid=grid)


def same_as_base(fmt, items, bs, max_units, grid=2, cached=False):
    rb, base = base_compress(fmt, items, bs, max_units, grid)
    r, b = eg.compress(fmt, items, bs, max_units, grid=grid, form=3, cached=cached)
    assert (rb, r) == (0, 0), "a kernel wrote in front of a window"
    n = len(items)
    assert [int(x) for x in b.status[:n]] == [int(x) for x in base.status[:n]]
    assert [int(x) for x in b.out_len[:n]] == [int(x) for x in base.out_len[:n]]
    assert [int(x) for x in b.result[:2]] == [int(x) for x in base.result[:2]]
    for i in range(n):
        assert b.window(i) == base.window(i), i
    assert int(b.result[3]) == 0
    nothing_behind(b)
    return b


def body_statuses(fmt):
    bs = 1000
    kinds = (lambda n, k: golden_bytes("plrabn12.txt")[k * 1000:k * 1000 + n], lambda n, k: datagen.lz_structured(n, k),
             lambda n, k: datagen.random_bytes(n, k), lambda n, k: datagen.zeros(n))
    plains = [kinds[k % 4](n, k) for k, n in enumerate((2500, 0, 999, 3001, 0, 1, 700))]         # 3 + 0 + 1 + 4 + 0 + 1 + 1 units
    wants = [want_of(fmt, p, bs) for p in plains]
    need = sum(-(-len(p) // bs) for p in plains)
    items = [(p, len(w)) for p, w in zip(plains, wants)]
    for max_units in (need, need - 1, 7, 4, 3, 0):
        step(fmt, "max units", max_units)
        b = same_as_base(fmt, items, bs, max_units)
        first = ok = 0
        for i, p in enumerate(plains):
            n = -(-len(p) // bs)
            if n and first + n > max_units:
                assert (int(b.status[i]), int(b.out_len[i])) == (rc.TOO_LARGE, 0) and b.window(i) == FILL * len(wants[i]), i
            else:
                ok += check_item(b, i, wants[i], len(wants[i]))                          # the items in front of the cut complete
            first += n
        done = sum(-(-len(p) // bs) for i, p in enumerate(plains) if int(b.status[i]) == rc.OK)
        assert [int(x) for x in b.result] == [need, ok, done if max_units else 0, 0], [int(x) for x in b.result]
    step(fmt, "a capacity one byte short")
    short = [(p, len(w) - 1 if i in (0, 3) else len(w)) for i, (p, w) in enumerate(zip(plains, wants))]
    b = same_as_base(fmt, short, bs, need, cached=True)
    assert [check_item(b, i, wants[i], short[i][1]) for i in range(len(plains))] == [i not in (0, 3) for i in range(len(plains))]
    assert [int(x) for x in b.result] == [need, len(plains) - 2, need, 0]
    step(fmt, "a null src, a null src of no bytes, src_len of 4 GiB, a null dst")
    bad = [(b"abc", 64, 1), (b"", 16, 1, 0), (b"abc", 64, 0, 1 << 32), (b"abcd" * 10, 0, 2), (plains[0], len(wants[0]))]
    b = same_as_base(fmt, bad, bs, 8)
    assert [int(x) for x in b.status[:5]] == [rc.INVALID, rc.OK, rc.TOO_LARGE, rc.DST_TOO_SMALL, rc.OK]
    assert int(b.out_len[3]) == len(want_of(fmt, b"abcd" * 10, bs)) and check_item(b, 4, wants[0], len(wants[0]))
    step(fmt, "no items")
    r, b = eg.compress(fmt, [], bs, 4, grid=1)
    assert r == 0 and [int(x) for x in b.result] == [0, 0, 0, 0]


BODIES = {f.__name__[5:]: f for f in (body_carriers, body_one_wavefront, body_statuses)}


def in_child(name, *args):
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import conftest, test_items_gt_emulated as t\n"
            "t.BODIES[sys.argv[2]](*[int(a) if a.lstrip('-').isdigit() else a for a in sys.argv[3:]])\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code, HERE, name] + [str(int(a)) if isinstance(a, bool) else str(a) for a in args], capture_output=True,
                         text=True, timeout=1500)
    lines = out.stdout.strip().splitlines()
    last = next((ln for ln in reversed(lines) if ln.startswith("step ")), "none")
    assert out.returncode == 0 and lines and lines[-1] == "ok", \
        ("status %d (negative: a signal, i.e. an access outside a guarded buffer) at %s" % (out.returncode, last), out.stderr[-2000:])


def test_sz_streams_of_the_alias_and_planted_inputs_show_the_parse():
    kc.assert_sz_inputs_stay_visible()


@pytest.mark.parametrize("cached", KINDS, ids=["slot_cache", "filter_alone"])
@pytest.mark.parametrize("form", kc.FORMS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_carrier_streams_are_the_oracles(fmt, form, cached):
    """Every call of k1_carrier_cases.raw_calls() / sz_calls() -- the inputs built to reach the edges of K1's strided scan and of
    its alias analysis, sources at every alignment -- in both forms of the parse behind both kinds of table: statuses, lengths
    and bytes equal the case's `wants` at the case's capacities, d_result = [units, items, units, 0]."""
    kc.assert_sz_inputs_stay_visible()
    in_child("carriers", fmt, form, cached)


@pytest.mark.parametrize("bs", [1, 256, 4096, 8192, 8193, 32768, 65535])
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_wavefront_takes_the_fragments_of_many_items(fmt, bs):
    """grid = 1: one wavefront's table serves, in turn, text, random bytes, zeros, a 1-byte item, the text again and the text off
    alignment; then the same call on the tables that run left.  Identical bytes, the oracle's."""
    in_child("one_wavefront", fmt, bs)


@pytest.mark.parametrize("fmt", FORMATS)
def test_statuses_are_the_base_calls(fmt):
    """The max-units cut in the middle of the batch, a capacity one byte short, a null src, src_len of 4 GiB, a null dst, no
    items: statuses, lengths, d_result[0..1] and every window equal the base call's emulator answers; no write in front of a
    window (rc 100) anywhere."""
    in_child("statuses", fmt)
