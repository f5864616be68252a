"""The case list of the reference differential: which inputs the reference's own codec was run on when
tests/golden/reference_digests.json was recorded (tools/record_reference.py), and how a test rebuilds each of them from
what is in the repository.  Used by the recording tool, tests/test_reference_differential.py (oracle, live reference and
wave emulator against the records) and tests/test_gpu_reference_digests.py (the GPU against the records).

A case id is a path of generator name and arguments; `input_for` / `stream_for` turn it back into bytes.  No input is
stored anywhere: the fixture holds ids, lengths, statuses and digests only."""
import functools
import json
import os

import numpy as np

import datagen
import oracle_lib as oracle
from conftest import GOLDEN_PAIRS, golden_bytes

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_digests.json")

# The edge matrix starts at block size 31: below it the per-block size words push streams of incompressible input past the
# reference's output allocation (ref_lib.in_reference_domain), where the reference has no defined output.
MATRIX_BLOCK_SIZES = datagen.BLOCK_SIZES + (31, 4097, 8192, 8193, 12345, 32767, 32769)
GOLDEN_BLOCK_SIZES = (255, 4097, 16384, 65535)
SLICE = 1 << 20
EMU_CUT = 40_000          # the emulator runs a lane per fiber: inputs are cut as tests/test_emulated_kernels.py cuts them


def _text():
    return golden_bytes("plrabn12.txt")


@functools.lru_cache(maxsize=1)
def _silesia_unit():
    import silesia_mix
    st, xml = oracle.decompress(golden_bytes("xml.snappy"))
    assert st == 0
    return silesia_mix.build_unit(np.frombuffer(xml, dtype=np.uint8), seed=0).tobytes()     # what bench.py compresses


@functools.lru_cache(maxsize=1)
def _edges():
    return dict(datagen.edge_cases(_text()))


@functools.lru_cache(maxsize=256)
def input_for(case_id):
    kind, _, rest = case_id.partition("/")
    if kind == "cut":                                        # cut/<bytes>/<inner case id>
        n, _, inner = rest.partition("/")
        return input_for(inner)[:int(n)]
    if kind == "edge":
        return _edges()[rest]
    if kind == "golden":
        return golden_bytes(rest + ".txt")
    if kind == "dickens":
        import standins
        return datagen.dickens_like(standins.prose_texts())
    if kind == "silesia":
        unit = _silesia_unit()
        start = {"start": 0, "middle": len(unit) // 2, "tail": (len(unit) - SLICE) | 1}[rest]   # tail: odd start, partial last block
        return unit[start:start + SLICE]
    args = [int(a) for a in rest.split("/")]
    if kind == "lz":
        return datagen.lz_structured(*args)                  # n, seed
    if kind == "records":
        return datagen.records(*args)                        # n, seed
    if kind == "lowent":
        return datagen.low_entropy(*args)                    # n, alphabet, seed
    if kind == "interleave":
        return datagen.text_random_interleave(_text(), *args)   # n, seed
    raise KeyError(case_id)


def _seeded(kind, count, seed0, extra=()):
    """Seeded lengths and block sizes for one generator: (case id, block size) pairs."""
    r = np.random.default_rng(seed0)
    out = []
    for k in range(count):
        n = int(r.integers(1, 300_000))
        args = [n] + [int(r.choice(e)) for e in extra] + [seed0 + k]
        cid = kind + "/" + "/".join(str(a) for a in args)
        for bs in sorted({int(b) for b in r.choice([31, 100, 700, 4096, 4097, 8192, 16384, 32768, 32769, 65535], size=2, replace=False)}):
            out.append((cid, bs))
    return out


# the slice the wave emulator runs (C.4): inputs cut to <= 40 kB, with records of their own
EMU_COMPRESS_CASES = (
    [("cut/%d/%s" % (EMU_CUT, inner), bs)
     for inner in ("golden/terror2", "edge/interleave", "edge/records", "edge/lowent", "lz/34000/7")
     for bs in (32768, 4097)] +
    [("cut/6000/%s" % inner, bs)
     for inner in ("edge/zeros100k", "edge/period2047", "edge/period1", "edge/period7", "edge/random200k", "golden/coding", "edge/text257",
                   "edge/text17", "edge/interleave")
     for bs in (65535, 700, 31)])


@functools.lru_cache(maxsize=1)
def compress_cases():
    """Every (case id, block size) the fixture records a reference stream for."""
    cases = [("edge/" + name, bs) for name in _edges() for bs in MATRIX_BLOCK_SIZES]
    cases += [("golden/" + name, bs) for name in GOLDEN_PAIRS for bs in GOLDEN_BLOCK_SIZES]
    cases += _seeded("lz", 10, 100) + _seeded("records", 6, 200) + _seeded("lowent", 6, 300, extra=([2, 4, 16, 64],)) + _seeded("interleave", 6, 400)
    cases += [("silesia/" + part, bs) for part in ("start", "middle", "tail") for bs in (32768, 65535)]
    cases += [("dickens/whole", bs) for bs in (32768, 65535)]
    cases += EMU_COMPRESS_CASES
    assert len(set(cases)) == len(cases)
    return tuple(cases)


# ---- decode cases --------------------------------------------------------------------------------------------------

ELEMENT_BLOCK_SIZES = (64, 700, 4097, 20000, 32768, 65535)


def element_cases():
    """elem/<total>/<block size>/<seed>/<flavour>: datagen.element_stream flavours 0-3 x six block sizes, a few blocks each
    with a partial last one (small enough for the emulator to decode all of them)."""
    out = []
    for flavour in range(4):
        for k, bs in enumerate(ELEMENT_BLOCK_SIZES):
            total = min(3 * bs + 17 + k, 9000 + 3777 * k) if bs < 20000 else bs + 5000 + 311 * k
            out.append("elem/%d/%d/%d/%d" % (total, bs, 3000 * flavour + k, flavour))
    return out


def damaged_element_streams(count, rng_seed=4242, sizes=(700, 4097, 32768), n_lo=2_000, n_hi=60_000, seed_base=9000):
    """The recipe of test_gpu_parity.test_decoder_agrees_with_oracle_on_damaged_element_streams: element streams with one
    to three bytes overwritten behind the header and the first size word.  -> list of (stream, header length, positions hit)."""
    r = np.random.default_rng(rng_seed)
    out = []
    for seed in range(count):
        bs = int(r.choice(list(sizes)))
        stream, _ = datagen.element_stream(int(r.integers(n_lo, n_hi)), bs, seed_base + seed, seed % 4)
        _, _, hdr = oracle.read_header(stream)
        b = bytearray(stream)
        hits = []
        for _ in range(int(r.integers(1, 4))):
            at = int(r.integers(hdr + 4, len(b)))
            b[at] = int(r.integers(0, 256))
            hits.append(at)
        out.append((bytes(b), hdr, hits))
    return out


DAMAGED_COUNT = 60


@functools.lru_cache(maxsize=1)
def _damaged60():
    return damaged_element_streams(DAMAGED_COUNT)


def decode_cases():
    return element_cases() + ["damaged/%d" % k for k in range(DAMAGED_COUNT)]


def is_damaged(case_id):
    return case_id.startswith("damaged/")


def stream_for(case_id):
    """-> (stream, plaintext or None): the plaintext of an element stream is known by construction."""
    kind, _, rest = case_id.partition("/")
    if kind == "damaged":
        return _damaged60()[int(rest)][0], None
    total, bs, seed, flavour = (int(a) for a in rest.split("/"))
    return datagen.element_stream(total, bs, seed, flavour)


# ---- the fixture -----------------------------------------------------------------------------------------------------

def load_fixture():
    """-> (compress records {(case id, block size): dict}, decode records {case id: dict}, the whole document)."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    comp = {(r[0], r[1]): dict(zip(doc["compress_columns"], r)) for r in doc["compress"]}
    dec = {r[0]: dict(zip(doc["decode_columns"], r)) for r in doc["decode"]}
    return comp, dec, doc
