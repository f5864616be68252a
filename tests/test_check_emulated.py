"""CPU tests of the check kernels (pim-compression_amd/csrc/snappy_check.hpp) on the lockstep wave emulator.  The yardstick is
the UNMODIFIED K2 on the same emulator (emu_lib.decompress_block, emu_raw_lib.decompress): the check must give K2's verdict
for every block and every raw stream, without an output buffer.  Every stream ends at an inaccessible page, so one byte read
behind it is a fault -- a legitimate failure here, which is why every body below runs in a child process that names the step
it is on."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emu_check_lib as ec
import emu_lib as emu
import emu_raw_lib as er
import k2_window_cases as kc
import oracle_lib as oracle
import raw_cases as rc
from conftest import golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))

# K2's own verdicts on the jobs of tests/k2_window_cases.py (OK, INVALID): both are amply present, so a check that always
# says one of them fails
K2_COUNTS = {"intact": (64, 0), "hand": (58, 276), "damaged": (374, 124)}


def step(*what):
    print("step", *what, flush=True)


# ---- per-block equivalence ----
def body_blocks(kind):
    jobs = {"intact": kc.intact_jobs, "hand": kc.hand_jobs, "damaged": lambda: kc.damaged_jobs(300)}[kind]()
    k2_ok = k2_invalid = 0
    for job in jobs:
        name, stream, at, out_len = job
        step(kind, name)
        k2, _ = emu.decompress_block(stream, at, out_len)
        got = ec.check_block(stream, at, out_len)
        print("verdicts", k2, got, flush=True)
        assert k2 in (ec.OK, ec.INVALID)
        assert got == k2, (name, got, k2)
        if kc.must_accept(job):
            assert got == ec.OK, name
        k2_ok += k2 == ec.OK
        k2_invalid += k2 == ec.INVALID
    print("K2 counts", k2_ok, k2_invalid, flush=True)
    assert (k2_ok, k2_invalid) == K2_COUNTS[kind], (k2_ok, k2_invalid)
    assert k2_ok + k2_invalid == len(jobs)


# ---- the batch path ----
def _offsets(stream):
    total, bs, offs = kc._offsets(stream)
    return total, bs, offs


def _k2_statuses(stream, total, bs, offs):
    return [emu.decompress_block(stream, at, min(bs, total - b * bs))[0] for b, at in enumerate(offs)]


def body_batch():
    by_bs = {}
    for name, stream, _ in kc.intact_containers():
        total, bs, offs = _offsets(stream)
        by_bs.setdefault(bs, (name, stream, total, offs))
    containers, want_status, want_result = [], [], []

    def add(c, statuses, result=None):
        containers.append(c)
        want_status.append(statuses)
        want_result.append(ec.fold(statuses) if result is None else result)

    for bs in (64, 4097, 65535):
        name, stream, total, offs = by_bs[bs]
        step("k2 on", name)
        add(ec.Container(stream, offs, total, bs), _k2_statuses(stream, total, bs, offs))
    add(ec.Container(oracle.compress(b"", 32768), [], 0, 32768), [])                      # an empty container
    # a damaged one: the 64-byte-block container with the first tag of blocks 1 and 3 turned into a copy (nothing to copy from
    # at the start of a block) and a byte changed somewhere in block 2 (whatever that does)
    name, stream, total, offs = by_bs[64]
    bad = bytearray(stream)
    assert len(offs) == 4
    bad[offs[1] + 4] = bad[offs[3] + 4] = 0xFF
    bad[offs[2] + 4 + 7] ^= 0x40
    bad = bytes(bad)
    step("k2 on the damaged container")
    damaged = _k2_statuses(bad, total, 64, offs)
    assert damaged[0] == ec.OK and damaged[1] == damaged[3] == ec.INVALID, damaged
    add(ec.Container(bad, offs, total, 64), damaged)
    # malformed descriptors: nothing of them is read (their streams are claimed longer than they are, their offsets point far
    # outside), nothing but their result words written
    junk = ec.lib().emu_check_status_junk()
    name, stream, total, offs = by_bs[4097]
    far = [1 << 40] * len(offs)
    oob = [ec.OUT_OF_BOUNDS, 0, ec.NONE, 0]
    add(ec.Container(stream, far, total, 4097, num_blocks=len(offs) + 1, stream_len=1 << 40, status_words=len(offs) + 1), [junk] * (len(offs) + 1), oob)
    add(ec.Container(stream, far, total, 0, num_blocks=len(offs), stream_len=1 << 40), [junk] * len(offs), oob)
    add(ec.Container(stream, far, total, 65536, num_blocks=1, stream_len=1 << 40, status_words=1), [junk], oob)
    add(ec.Container(stream, offs, total, 4097, flags=2), [junk] * len(offs), oob)           # blocks, no offsets
    add(ec.Container(stream, offs, total, 4097, flags=1), [junk] * len(offs), oob)           # bytes, no stream
    assert len(containers) >= 6

    for grid in (1, 3):
        for mode in (0, 1, 2):
            step("batch grid", grid, "status mode", mode)
            rcode, results, statuses = ec.check_blocks(containers, status_mode=mode, grid=grid)
            assert rcode == 0, "a word beside the results (1) or a status array (2) was written: %d" % rcode
            assert results == want_result, (results, want_result)
            if mode == 2:
                assert statuses == want_status
            else:
                assert all(s == [junk] * len(s) for s in statuses)
    step("no containers")
    assert ec.check_blocks([], grid=1)[0] == 0
    step("no wavefronts: the plan alone initialises every result")
    rcode, results, _ = ec.check_blocks(containers, grid=0)
    assert rcode == 0 and results == [[ec.OK if w[0] != ec.OUT_OF_BOUNDS else w[0], 0, ec.NONE, 0] for w in want_result]


def body_planner_trips():
    conts = kc.planner_trip_containers()
    k2 = {}
    for stream, offs, total, bs in conts:
        if stream not in k2:
            step("k2 on a container of", len(offs))
            k2[stream] = _k2_statuses(stream, total, bs, offs)
    want = [k2[c[0]] for c in conts]
    assert len(conts) > 1024 and want[1024] == [ec.OK, ec.OK, ec.INVALID, ec.OK], want[1024]
    assert sum(w == [ec.INVALID] for w in want) > 90 and sum(w == [ec.INVALID] for w in want[1025:]) > 0
    step("check", len(conts), "containers")
    rcode, results, statuses = ec.check_blocks([ec.Container(s, offs, total, bs) for s, offs, total, bs in conts], grid=3)
    assert rcode == 0
    for i, w in enumerate(want):
        assert statuses[i] == w and results[i] == ec.fold(w), (i, statuses[i], results[i], w)


# ---- raw ----
def _raw_decode(s):
    """the emulated decoder's (status, out_len) at full capacity, or None where it cannot be run (a length nobody can allocate)"""
    h = rc.header_parses(s)
    n = h[0] if h else 0
    if n > (1 << 22):
        return None
    _, b = er.decompress([(s, n)], grid=1)
    return int(b.status[0]), int(b.out_len[0])


def body_raw():
    cases = [("intact " + k, v) for k, v in rc.intact_vectors().items()] + [("damaged " + k, v) for k, v in rc.damaged_vectors().items()] + \
        [("fixture " + k, rc.fixture_stream(k)) for k in rc.FIXTURES]
    assert len(rc.intact_vectors()) == 13 and len(rc.damaged_vectors()) == 23 and len(rc.FIXTURES) == 6
    for name, s in cases:
        step("raw", name)
        got = ec.raw_check([s], grid=1)[0]
        assert got == rc.expect(s)[:2], (name, got, rc.expect(s)[:2])
        if name.startswith("damaged"):
            assert got[0] == rc.INVALID, name
        else:
            assert got[0] == rc.OK, name
        dec = _raw_decode(s)
        assert dec is not None and got == dec, (name, got, dec)
    s = rc.intact_vectors()["all_types"]
    n = rc.header_parses(s)[0]
    step("null src")
    assert ec.raw_check([(s, 1)], grid=1) == [(rc.INVALID, 0)]
    assert er.decompress([(s, n, 1)], grid=1)[1].status[0] == rc.INVALID
    step("src_len beyond the maximum")
    assert ec.raw_check([(s, 0, rc.RAW_MAX_LEN + 1)], grid=1) == [(rc.TOO_LARGE, n)]
    step("header beyond the maximum")
    big = rc.varint(rc.RAW_MAX_LEN + 1) + rc.literal(b"x")
    assert ec.raw_check([big], grid=1) == [rc.expect(big)[:2]] == [(rc.TOO_LARGE, rc.RAW_MAX_LEN + 1)]
    step("the largest header that is not too large")
    most = rc.varint(rc.RAW_MAX_LEN) + rc.literal(b"x")
    assert ec.raw_check([most], grid=1) == [(rc.INVALID, rc.RAW_MAX_LEN)]
    step("all in one launch of two wavefronts")
    streams = [s for _, s in cases]
    assert ec.raw_check(streams, grid=2) == [rc.expect(s)[:2] for s in streams]
    step("no items")
    assert ec.raw_check([], grid=1) == []


# ---- seeded mutation fuzz ----
FUZZ_SEED = 20240611
FUZZ_BLOCKS, FUZZ_RAW = 400, 100


def fuzz_cases():
    """500 single-byte mutations and truncations: 400 of terror2's four blocks (each as a stream of its own: size word and
    elements, the mutation anywhere in them), 100 of its raw fixture (behind the three header bytes, so that the decoder's
    output stays 105,438 bytes).  One in five is a truncation."""
    r = np.random.default_rng(FUZZ_SEED)
    framed = golden_bytes("terror2.snappy")
    total, bs, offs = kc._offsets(framed)
    ends = offs[1:] + [len(framed)]
    cases = []
    for k in range(FUZZ_BLOCKS):
        b = int(r.integers(0, len(offs)))
        block = bytearray(framed[offs[b]:ends[b]])
        if k % 5 == 4:
            block = block[:int(r.integers(0, len(block)))]
        else:
            block[int(r.integers(0, len(block)))] ^= int(r.integers(1, 256))
        cases.append(("block", bytes(block), min(bs, total - b * bs)))
    raw = rc.fixture_stream("terror2")
    for k in range(FUZZ_RAW):
        s = bytearray(raw)
        if k % 5 == 4:
            s = s[:int(r.integers(3, len(s)))]
        else:
            s[int(r.integers(3, len(s)))] ^= int(r.integers(1, 256))
        cases.append(("raw", bytes(s), total))
    return cases


def body_fuzz():
    cases = fuzz_cases()
    assert len(cases) == 500
    ok = invalid = 0
    for k, (kind, s, out_len) in enumerate(cases):
        step("fuzz", k, kind)
        if kind == "block":
            dec = emu.decompress_block(s, 0, out_len)[0]
            got = ec.check_block(s, 0, out_len)
        else:
            dec = _raw_decode(s)
            got = ec.raw_check([s], grid=1)[0]
            assert dec[1] == out_len
        assert got == dec, (k, kind, got, dec)
        st = dec if kind == "block" else dec[0]
        ok += st == ec.OK
        invalid += st == ec.INVALID
    print("decoder verdicts", ok, invalid, flush=True)
    assert ok + invalid == 500 and ok >= 50 and invalid >= 50, (ok, invalid)


BODIES = {f.__name__[5:]: f for f in (body_blocks, body_batch, body_raw, body_fuzz, body_planner_trips)}


def in_child(name, *args):
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import conftest, test_check_emulated as t\n"
            "t.BODIES[sys.argv[2]](*sys.argv[3:])\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code, HERE, name] + [str(a) for a in args], capture_output=True, text=True, timeout=1500)
    lines = out.stdout.strip().splitlines()
    last = next((ln for ln in reversed(lines) if ln.startswith("step ")), "none")
    assert out.returncode == 0 and lines and lines[-1] == "ok", \
        ("status %d (negative: a signal, i.e. an access outside a guarded buffer) at %s" % (out.returncode, last), out.stderr[-2000:])
    return lines


@pytest.mark.parametrize("kind", ["intact", "hand", "damaged"])
def test_every_block_gets_k2s_verdict(kind):
    """Every job of k2_window_cases.intact_jobs(), hand_jobs() and damaged_jobs(300): check status == K2 status, K2's own
    counts as recorded (64 / 0, 58 / 276, 374 / 124), blocks that are valid by construction OK."""
    lines = in_child("blocks", kind)
    assert "K2 counts %d %d" % K2_COUNTS[kind] in lines


def test_batch_of_mixed_containers_with_fewer_wavefronts_than_blocks():
    """check_plan_kernel + check_kernel, grids of 1 and 3 wavefronts: block sizes 64, 4097 and 65535, an empty container, a
    damaged one and five malformed descriptors in one call; without status arrays, with null ones, with all of them; counts
    and first-bad indices against a fold over K2's statuses; junk in and guards beside every array."""
    in_child("batch")


def test_more_containers_than_one_trip_of_the_planner():
    """1,031 containers, the 1,025th with four blocks of which one is damaged, damaged one-block containers on both sides of
    the planner's trip boundary: results and statuses against K2 per block."""
    in_child("planner_trips")


def test_raw_streams_get_the_decoders_verdict_and_length():
    in_child("raw")


def test_seeded_mutations_and_truncations_of_terror2():
    """500 mutations: the check equals the emulated decoder on every one, and the decoder alone gives at least 50 of each
    verdict."""
    in_child("fuzz")
