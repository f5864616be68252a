#!/usr/bin/env python3
"""Regenerates tests/golden/reference_digests.json from the live reference binary (oracle/_ref/dpu_snappy_ref, built by
`make -C oracle ref`): for every case of tests/reference_cases.py the reference's exit status, the length and SHA-256 of
what it wrote.  The file holds recorded results only -- case ids, lengths, statuses, digests.

    python tools/record_reference.py            write the fixture
    python tools/record_reference.py --check    regenerate in memory and compare with the committed file

Refuses to write if any compress record lies outside ref_lib.in_reference_domain (there the reference overruns its output
allocation and what it writes is not a specification), or if the file would exceed 256 KiB."""
import hashlib
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pim-compression_amd")):
    sys.path.insert(0, p)

import oracle_lib as oracle          # noqa: E402
import ref_lib                       # noqa: E402
import reference_cases as rc         # noqa: E402

MAX_BYTES = 256 * 1024
COMPRESS_COLUMNS = ["case", "block_size", "n", "status", "stream_len", "sha256"]
DECODE_COLUMNS = ["case", "status", "sha256"]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def compress_record(case):
    cid, bs = case
    data = rc.input_for(cid)
    st, stream = ref_lib.compress(data, bs)
    if st != 0:
        return [cid, bs, len(data), st, None, None]
    return [cid, bs, len(data), 0, len(stream), sha(stream)]


def decode_record(cid):
    stream, _ = rc.stream_for(cid)
    st, plain = ref_lib.decompress(stream, timeout=30)
    return [cid, st, sha(plain) if st == 0 else None]


def oracle_accepts(stream):
    try:
        st, out = oracle.decompress(stream)
    except ValueError:
        return False, None
    return st == 0, out


def generate():
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        comp = list(pool.map(compress_record, rc.compress_cases()))
        dec = list(pool.map(decode_record, rc.decode_cases()))
    outside = [(r[0], r[1]) for r in comp if r[3] != 0 or not ref_lib.in_reference_domain(r[2], r[4])]
    if outside:
        raise SystemExit("refusing: %d compress records failed or lie outside the reference's domain, e.g. %r" % (len(outside), outside[:5]))
    # damaged streams on which oracle and reference disagree about acceptance (the oracle refuses reads outside the block):
    # counted here, asserted as an exact count by the tests, so that a drift in either direction shows
    disagree = []
    for cid, st, digest in dec:
        if rc.is_damaged(cid) and st >= 0:
            ok, _ = oracle_accepts(rc.stream_for(cid)[0])
            if ok != (st == 0):
                disagree.append(cid)
    return {
        "about": "Results of the reference's own host codec on the cases of tests/reference_cases.py; written by tools/record_reference.py",
        "compress_columns": COMPRESS_COLUMNS,
        "decode_columns": DECODE_COLUMNS,
        "damaged_acceptance_disagreements": len(disagree),
        "damaged_acceptance_disagreement_cases": disagree,
        "compress": comp,
        "decode": dec,
    }


def render(doc):
    lines = ["{"]
    for k in ("about", "compress_columns", "decode_columns", "damaged_acceptance_disagreements", "damaged_acceptance_disagreement_cases"):
        lines.append(" %s: %s," % (json.dumps(k), json.dumps(doc[k])))
    for k in ("compress", "decode"):
        lines.append(" %s: [" % json.dumps(k))
        lines.append(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in doc[k]))
        lines.append(" ]" + ("," if k == "compress" else ""))
    lines.append("}")
    return "\n".join(lines) + "\n"


def main():
    if not ref_lib.available():
        raise SystemExit("no reference binary: " + ref_lib.MAKE_TARGET)
    text = render(generate())
    if len(text) > MAX_BYTES:
        raise SystemExit("refusing: the fixture would take %d bytes (limit %d)" % (len(text), MAX_BYTES))
    if "--check" in sys.argv[1:]:
        with open(rc.FIXTURE) as f:
            same = f.read() == text
        print("fixture %s" % ("identical" if same else "DIFFERS from what the reference binary gives now"))
        return 0 if same else 1
    with open(rc.FIXTURE, "w") as f:
        f.write(text)
    print("wrote %s: %d bytes" % (os.path.relpath(rc.FIXTURE, ROOT), len(text)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
