#!/usr/bin/env python3
"""Record the third-party raw Snappy streams the raw-format tests decode: tests/golden/raw/NAME.raw_snappy, made with Apache
Arrow's Snappy codec (pyarrow; it links Google's Snappy) from the committed plaintexts and the seeded generators of
tests/datagen.py, plus tests/golden/raw/fixtures.json with the lengths and SHA-256 of plaintext and stream.

Usage: python tools/record_raw_fixtures.py            write the fixtures (needs pyarrow)
       python tools/record_raw_fixtures.py --check    compare the committed files with the JSON and, where pyarrow is
                                                      importable, decode them with it and compare with the plaintexts
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raw_cases as rc   # noqa: E402


def sha(b):
    return hashlib.sha256(b).hexdigest()


def record():
    import pyarrow as pa
    codec = pa.Codec("snappy")
    os.makedirs(rc.FIXTURE_DIR, exist_ok=True)
    meta = {}
    for name in rc.FIXTURES:
        plain = rc.fixture_plain(name)
        s = codec.compress(plain, asbytes=True)
        assert rc.trs.decode_raw(s) == plain, name
        with open(os.path.join(rc.FIXTURE_DIR, name + ".raw_snappy"), "wb") as f:
            f.write(s)
        meta[name] = {"plain_len": len(plain), "plain_sha256": sha(plain), "stream_len": len(s), "stream_sha256": sha(s),
                      "made_with": "pyarrow " + pa.__version__}
        print(f"{name}: {len(plain)} -> {len(s)}")
    with open(os.path.join(rc.FIXTURE_DIR, "fixtures.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


def check():
    with open(os.path.join(rc.FIXTURE_DIR, "fixtures.json")) as f:
        meta = json.load(f)
    try:
        import pyarrow as pa
        codec = pa.Codec("snappy")
    except ImportError:
        codec = None
    for name in rc.FIXTURES:
        s = rc.fixture_stream(name)                  # (asserts length and digest of the stream)
        plain = rc.fixture_plain(name)
        m = meta[name]
        assert (len(plain), sha(plain)) == (m["plain_len"], m["plain_sha256"]), name
        assert rc.trs.decode_raw(s) == plain, name
        if codec is not None:
            assert codec.decompress(s, decompressed_size=len(plain), asbytes=True) == plain, name
        print(f"{name}: ok" + ("" if codec else " (pyarrow not importable: digests and the Python decoder only)"))


if __name__ == "__main__":
    check() if "--check" in sys.argv[1:] else record()
