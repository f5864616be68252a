"""What pins what: the reference's own host codec (oracle/_ref/dpu_snappy_ref, built from the reference checkout where
there is one) -> tests/golden/reference_digests.json (its recorded results, tools/record_reference.py) -> the oracle, the
wave emulator and (tests/test_gpu_reference_digests.py) the GPU.  The first test needs neither the binary nor the
reference checkout and runs on every machine; the live ones skip where the binary is absent.

The domain rule: the reference writes the whole stream into ONE allocation of 32 + n + n / 6 bytes
(ref_lib.in_reference_domain); a stream longer than that -- tiny blocks, whose 4-byte size words dominate -- is written
past it and the reference's output is undefined (right length, zeros or garbage behind some point, or a crash).  There
the oracle is the specification, and a comparison with the reference may leave a case out for that reason ONLY."""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import datagen
import oracle_lib as oracle
import ref_lib
import reference_cases as rc
from conftest import golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
NEEDS_BINARY = pytest.mark.skipif(not ref_lib.available(), reason="no oracle/_ref/dpu_snappy_ref: build it with `%s`" % ref_lib.MAKE_TARGET)


def sha(b):
    return hashlib.sha256(b).hexdigest()


def _oracle_decode(stream):
    try:
        return oracle.decompress(stream)
    except ValueError:
        return 1, None


# ---- 1. the oracle against the recorded reference: every machine ----------------------------------------------------

def test_fixture_covers_the_case_list_and_lies_inside_the_reference_domain():
    comp, dec, doc = rc.load_fixture()
    assert set(comp) == set(rc.compress_cases()) and len(doc["compress"]) == len(comp)
    assert set(dec) == set(rc.decode_cases()) and len(doc["decode"]) == len(dec)
    assert os.path.getsize(rc.FIXTURE) <= 256 * 1024
    outside = [k for k, r in comp.items() if r["status"] != 0 or not ref_lib.in_reference_domain(r["n"], r["stream_len"])]
    assert not outside                                       # 0 % of the fixture is left out of any comparison
    # not only the 32 KiB text goldens: most records are other block sizes and other kinds of data
    assert sum(1 for (_, bs) in comp if bs != 32768) >= 700
    assert any(r["n"] > (1 << 20) for r in comp.values())


def test_oracle_compress_equals_every_reference_record():
    comp, _, _ = rc.load_fixture()
    wrong = []
    for (cid, bs), rec in comp.items():
        data = rc.input_for(cid)
        assert len(data) == rec["n"], (cid, "the generators no longer give the recorded input")
        stream = oracle.compress(data, bs)
        if len(stream) != rec["stream_len"] or sha(stream) != rec["sha256"]:
            wrong.append((cid, bs, len(stream), rec["stream_len"]))
    assert not wrong, (len(wrong), wrong[:10])


def test_oracle_decode_against_every_reference_record():
    _, dec, doc = rc.load_fixture()
    disagree, both = [], 0
    for cid, rec in dec.items():
        stream, plain = rc.stream_for(cid)
        st, out = _oracle_decode(stream)
        if not rc.is_damaged(cid):
            assert rec["status"] == 0 and rec["sha256"] == sha(plain), cid      # the reference decodes every valid element stream
            assert st == 0 and out == plain, cid
            continue
        if rec["status"] < 0:
            continue                                         # the reference ended on a signal: nothing to compare
        ref_ok = rec["status"] == 0
        if st == 0:
            assert ref_ok, (cid, "the oracle accepts what the reference rejected")
            assert sha(out) == rec["sha256"], cid
            both += 1
        elif ref_ok:
            disagree.append(cid)                             # the oracle refuses reads outside the block; the reference does not
    assert both > 0
    assert len(disagree) == doc["damaged_acceptance_disagreements"], disagree
    assert disagree == doc["damaged_acceptance_disagreement_cases"]


# ---- 2. the live reference: the fixture is not stale, and a wider sweep that is not recorded ----------------------------

def _pool():
    return ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))


@NEEDS_BINARY
def test_live_reference_reproduces_every_record():
    comp, dec, _ = rc.load_fixture()

    def one_compress(item):
        (cid, bs), rec = item
        st, stream = ref_lib.compress(rc.input_for(cid), bs)
        return None if (st == 0 and len(stream) == rec["stream_len"] and sha(stream) == rec["sha256"]) else (cid, bs, st)

    def one_decode(item):
        cid, rec = item
        st, plain = ref_lib.decompress(rc.stream_for(cid)[0], timeout=30)
        return None if (st == rec["status"] and (st != 0 or sha(plain) == rec["sha256"])) else (cid, st)

    with _pool() as pool:
        stale = [x for x in pool.map(one_compress, comp.items()) if x] + [x for x in pool.map(one_decode, dec.items()) if x]
    assert not stale, (len(stale), stale[:10], "re-record with tools/record_reference.py if the reference changed")


SWEEP_CASES = 1040
SWEEP_BLOCK_SIZES = sorted({31, 65535} | {p + d for k in range(5, 17) for p in (1 << k,) for d in (-1, 0, 1) if 31 <= p + d <= 65535})


def sweep_cases():
    """Seeded (generator, arguments, block size): half the block sizes from the powers of two and their neighbours, half
    anywhere in 31..65535."""
    r = np.random.default_rng(20261016)
    text = golden_bytes("plrabn12.txt")
    edges = datagen.edge_cases(text)
    gens = [lambda n, s: datagen.lz_structured(n, s), lambda n, s: datagen.records(n, s),
            lambda n, s: datagen.low_entropy(n, int(2 ** (1 + s % 6)), s), lambda n, s: datagen.text_random_interleave(text, n, s),
            lambda n, s: edges[s % len(edges)][1][:n]]
    for k in range(SWEEP_CASES):
        n = int(r.integers(1, 3000)) if k % 4 == 0 else int(r.integers(1, 150_000))
        bs = int(r.choice(SWEEP_BLOCK_SIZES)) if k % 2 else int(r.integers(31, 65536))
        yield k, gens[k % len(gens)](n, 7000 + k), bs


@NEEDS_BINARY
def test_live_reference_sweep_oracle_against_binary():
    def one(case):
        k, data, bs = case
        ours = oracle.compress(data, bs)
        if not ref_lib.in_reference_domain(len(data), len(ours)):
            return "outside"                                  # the ONLY reason a case may be left out
        st, theirs = ref_lib.compress(data, bs)
        if st != 0 or theirs != ours:
            return (k, len(data), bs, st)
        st, back = ref_lib.decompress(ours)                  # and the reference reads the oracle's stream back
        return None if (st == 0 and back == data) else (k, len(data), bs, "decode", st)

    with _pool() as pool:
        results = list(pool.map(one, sweep_cases()))
    assert len(results) >= 1000
    wrong = [x for x in results if x not in (None, "outside")]
    assert not wrong, (len(wrong), wrong[:10])
    assert results.count("outside") <= len(results) // 20    # at most 5 % of the sweep


# ---- 3. outside the domain the oracle is the specification --------------------------------------------------------------

def test_outside_the_reference_domain_the_oracle_is_the_specification():
    """coding.txt at block size 7: 4 size bytes + 1 tag for every 7 bytes of text.  The stream exceeds what the reference
    allocates for it; the library grows its buffer there (tests/test_gpu_parity.py), and the oracle round-trips.  What the
    reference makes of it is undefined: observed were a stream of the right length with zeros or garbage from about byte
    11,040 on, and SIGSEGV for 70 kB at block size 1 -- so, live, only `not the oracle's stream, or no stream` is asserted."""
    data = golden_bytes("coding.txt")
    stream = oracle.compress(data, 7)
    assert len(stream) > 32 + len(data) + len(data) // 6
    assert not ref_lib.in_reference_domain(len(data), len(stream))
    st, back = oracle.decompress(stream)
    assert st == 0 and back == data
    if ref_lib.available():
        st, theirs = ref_lib.compress(data, 7)
        assert st != 0 or theirs != stream
    # and the boundary of the rule itself (snappy_compress.c:55-57, dpu_snappy.h:18)
    assert ref_lib.in_reference_domain(6, 39) and not ref_lib.in_reference_domain(6, 40)
    assert ref_lib.in_reference_domain(30 << 20, 1) and not ref_lib.in_reference_domain((30 << 20) + 1, 1)


# ---- 4. the wave emulator against the reference's records ------------------------------------------------------------------

_EMU_SLICE = """
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import emu_lib as emu, oracle_lib as oracle, reference_cases as rc
comp, dec, _ = rc.load_fixture()
sha = lambda b: hashlib.sha256(b).hexdigest()
for cid, bs in rc.EMU_COMPRESS_CASES:
    rec, data = comp[(cid, bs)], rc.input_for(cid)
    for cv in (43503, 3501):                      # the product's global-table and LDS-table kernels, stream form
        got = emu.compress(data, bs, cv)
        assert len(got) == rec["stream_len"] and sha(got) == rec["sha256"], (cid, bs, cv)
for cid in rc.element_cases():
    stream, plain = rc.stream_for(cid)
    total, bs, hdr = oracle.read_header(stream)
    st, out = emu.decompress(stream, total, bs, hdr)
    assert st == 0 and sha(out) == dec[cid]["sha256"], cid
print("ok")
"""


def test_emulated_kernels_equal_the_reference_records():
    """K1 (variants 43503 and 3501) and K2 under the wave emulator against what the REFERENCE gave for the same (cut)
    inputs -- the oracle is not consulted.  In a child process: the emulator guards K2's buffers with inaccessible pages."""
    out = subprocess.run([sys.executable, "-c", _EMU_SLICE, HERE], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stderr[-2000:])
