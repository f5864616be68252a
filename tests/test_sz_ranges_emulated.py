"""CPU tests of the .sz index and range calls: the UNMODIFIED kernels of pim-compression_amd/csrc/snappy_sz_ranges.hpp (behind the
split walk's, as snappy_hip_sz_index_batch enqueues them) on the lockstep wave emulator, every case of tests/sz_ranges_cases.py at
grids 1 and 3, the scratch with exactly one slot and with one slot per workgroup.  Every dst is a window of exactly the range's
length between inaccessible pages and every src ends at one, so one byte written outside a window or read behind a stream is a
fault -- a legitimate failure here, which is why every body runs in a child process that names the step it is on.

Yardsticks, none the code under test: the Python model of sz_ranges_cases (statuses, bad chunks, every window byte; an
out-of-bounds range leaves its window at the fill), the SzChunk records of the split call's kernels in emu_sz_split_lib (the
index's records word for word but for the reserved word), and the model's chain verdict (the index statuses).  Every item of the
index call has a null dst and a capacity of 0: the property the shadow items exist for.  All comparisons are exact."""
import os
import subprocess
import sys

import pytest

import emu_sz_ranges_lib as esr
import emu_sz_split_lib as ess
import sz_ranges_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = bytes([esr.FILL])
SEGMENT, MAX_SEGMENTS = 1024, 512


def step(*what):
    print("step", *what, flush=True)


def words_of(rec, item):
    """the 8 words of a snappy_hip_sz_chunk from the model's record"""
    src_off, dst_off, info, ulen = rec[:4]
    return (src_off & 0xffffffff, src_off >> 32, dst_off & 0xffffffff, dst_off >> 32, info & 0xffffffff, ulen, item, 0)


def check_ranges(name, o, ranges, want):
    for r, (w, q) in enumerate(zip(want, ranges)):
        got = (int(o.status[r]), int(o.bad_chunk[r]))
        assert got == w[:2], (name, r, q, got, w[:2])
        if w[0] == cases.OK:
            assert o.window(r) == w[2], (name, r, q)
        elif w[0] == cases.OUT_OF_BOUNDS:
            assert o.window(r) == FILL * len(o.window(r)), (name, r, q)


def body_case(name, grid, slots):
    c = cases.case(name)
    streams = [s for _, s in c.streams]
    idx, want = cases.expected(c)
    models = [cases.index_model(s) for s in streams]
    need = sum(len(m[1]) for m in models)
    step(name, "grid", grid, "slots", slots, ": index and ranges")
    rc, o = esr.run(streams, need + 3, SEGMENT, MAX_SEGMENTS, c.ranges, flags=0 if c.verify else 1, grid=grid, slots=slots)
    assert rc == 0, "a kernel wrote in front of a window (100) or behind a scratch (101): %d" % rc
    assert [int(x) for x in o.idx_status[:len(streams)]] == idx, name
    assert [int(x) for x in o.result[:2]] == [need, idx.count(cases.OK)], (name, o.result)
    at = 0
    for i, (st, recs, total) in enumerate(models):
        assert o.descs[i] == (1, len(streams[i]), at if recs else o.descs[i][2], len(recs), total), (name, i, o.descs[i])
        for k, rec in enumerate(recs):
            assert o.records[at + k] == words_of(rec, i), (name, i, k)
        at += len(recs)
    step(name, ": the split call's records")
    r0, b = ess.decompress([(s, m[2]) for s, m in zip(streams, models)], need + 3, SEGMENT, MAX_SEGMENTS, flags=1, grid=grid)
    assert r0 == 0 and len(b.records) == len(o.records) == need
    assert [r[:7] for r in b.records] == [r[:7] for r in o.records] and all(r[7] == 0 for r in o.records), name
    # ([1] differs by design: the items indexed OK, not the items decoded OK)
    assert [int(b.result[j]) for j in (0, 2, 3)] == [int(o.result[j]) for j in (0, 2, 3)], (name, b.result, o.result)
    check_ranges(name, o, c.ranges, want)


def body_stale(grid):
    label, s, k, rs = cases.stale_case()
    st, recs, total = cases.index_model(s)
    _, chunks, _ = cases.chain(s)
    ranges = [(0, off, n, False) for off, n in rs]
    for name, edit in cases.stale_edits().items():
        step("stale", name, "grid", grid)
        r = dict(zip(("src_off", "dst_off", "info", "ulen", "item"), recs[k]))
        edit(r)
        words = words_of((r["src_off"], r["dst_off"], r["info"], r["ulen"]), 0)
        rc, o = esr.run([s], len(recs), SEGMENT, MAX_SEGMENTS, ranges, grid=grid, edits=[(k, words)])
        assert rc == 0
        want = []
        for off, n in rs:
            first, last = cases.touched(chunks, off, n)
            want.append((cases.INVALID, k, None) if first <= k <= last else cases.range_model(s, off, n))
        check_ranges(("stale", name), o, ranges, want)


def body_limits():
    s = cases.streams()["mixed_20k"][0]
    st, recs, total = cases.index_model(s)
    step("no items, no ranges")
    rc, o = esr.run([], 4, SEGMENT, 8, [])
    assert rc == 0 and [int(x) for x in o.result[:4]] == [0, 0, 0, 0]
    step("a null src beside a good item; max_chunks one short for the second good item")
    rc, o = esr.run([s, b"", s], 2 * len(recs) - 1, SEGMENT, MAX_SEGMENTS, [(0, 0, total, False), (1, 0, 1, False), (2, 0, 1, False), (2, 0, 0, False)],
                    null_src=(1,))
    assert rc == 0 and [int(x) for x in o.idx_status[:3]] == [cases.OK, cases.INVALID, cases.TOO_LARGE]
    assert o.descs[1][3:] == (0, 0) and o.descs[2][3:] == (0, 0) and int(o.result[0]) == 2 * len(recs) and int(o.result[1]) == 1
    assert [int(x) for x in o.status[:4]] == [cases.OK, cases.OUT_OF_BOUNDS, cases.OUT_OF_BOUNDS, cases.OK]
    assert o.window(0) == cases.streams()["mixed_20k"][1]
    step("no segments: every item walked serially")
    rc, o = esr.run([s], len(recs), SEGMENT, 0, [(0, 5, total - 9, False)])
    assert rc == 0 and int(o.status[0]) == cases.OK and o.window(0) == cases.streams()["mixed_20k"][1][5:total - 4]
    assert o.records == [words_of(r, 0) for r in recs] and [int(x) for x in o.result[2:4]] == [0, 1]


BODIES = {"case": body_case, "stale": body_stale, "limits": body_limits}


def in_child(body, *args):
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import conftest, test_sz_ranges_emulated as t\n"
            "t.BODIES[sys.argv[2]](*[int(a) if a.isdigit() else a for a in sys.argv[3:]])\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code, HERE, body] + [str(a) for a in args], capture_output=True, text=True, timeout=1500)
    lines = out.stdout.strip().splitlines()
    last = next((ln for ln in reversed(lines) if ln.startswith("step ")), "none")
    assert out.returncode == 0 and lines and lines[-1] == "ok", \
        ("status %d (negative: a signal, i.e. an access outside a guarded buffer) at %s" % (out.returncode, last), out.stderr[-3000:])


@pytest.mark.parametrize("grid,slots", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("name", cases.case_names())
def test_index_and_ranges_give_the_models_answers(name, grid, slots):
    in_child("case", name, grid, slots)


@pytest.mark.parametrize("grid", [1, 3])
def test_a_stale_record_is_invalid_for_the_ranges_that_touch_it(grid):
    in_child("stale", grid)


def test_limits_null_items_and_the_serial_walk():
    in_child("limits")
