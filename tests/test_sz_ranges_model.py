"""The model of tests/sz_ranges_cases.py against the strict reader sz_cases.read_sz (CPU): for every intact stream 200 seeded
ranges equal the slice of read_sz's plaintext, the whole-stream range has read_sz's verdict for every damaged stream whose chain
parses, the index model's records tile the stream, and the seeded cases hold what they promise."""
import random

import sz_cases as sz
import sz_ranges_cases as cases


def _intact():
    v = dict(sz.intact_streams())
    v.update(cases.streams())
    return v


def test_seeded_ranges_are_slices_of_the_readers_plaintext():
    for name, (s, plain) in _intact().items():
        st, n, got, bad = sz.read_sz(s)
        assert (st, got) == (sz.OK, plain), name
        rng = random.Random(len(s))
        for _ in range(200):
            off = rng.randrange(n + 1)
            length = rng.randint(0, n - off)
            for verify in (True, False):
                assert cases.range_model(s, off, length, verify) == (cases.OK, cases.NONE, plain[off:off + length]), (name, off, length)
        assert cases.range_model(s, n, 1)[0] == cases.OUT_OF_BOUNDS and cases.range_model(s, 1, n)[0] == cases.OUT_OF_BOUNDS
        assert cases.range_model(s, cases.U64 - 1, 1)[0] == cases.OUT_OF_BOUNDS


def test_the_whole_stream_range_has_the_readers_verdict():
    seen = set()
    for name, s in cases.parsing_damage().items():
        for verify in (True, False):
            st, n, plain, bad = sz.read_sz(s, verify=verify)
            if n == 0:
                continue
            got = cases.range_model(s, 0, n, verify)
            # an empty bad chunk at the range's first byte lies in front of `first`: the one kind a range cannot touch
            if name == "zero_varint_with_elements":
                assert st == sz.INVALID and bad == 0 and got[0] == cases.OK
                continue
            assert got[:2] == (st, bad), (name, verify, got[:2], (st, bad))
            if st == sz.OK:
                assert got[2] == plain
            seen.add(st)
    assert seen == {sz.OK, sz.INVALID, sz.CRC_MISMATCH}
    for name, s in sz.damaged_streams().items():
        if name not in cases.parsing_damage():
            assert cases.index_model(s) == (sz.read_sz(s)[0], [], 0), name
            assert sz.read_sz(s)[0] in (sz.INVALID, sz.UNSUPPORTED), name


def test_the_index_models_records_tile_the_stream():
    for name, (s, plain) in _intact().items():
        st, recs, total = cases.index_model(s)
        assert st == sz.OK and total == len(plain), name
        at = 0
        for src_off, dst_off, info, ulen, item in recs:
            L, hdr, compressed = info & 0xffffff, (info >> 24) & 15, (info >> 28) & 1
            assert dst_off == at and s[src_off] == (0 if compressed else 1) and int.from_bytes(s[src_off + 1:src_off + 4], "little") == L, name
            assert (hdr > 0) == bool(compressed) and ulen <= 65536
            at += ulen
        assert at == total


def test_the_seeded_cases_hold_what_they_promise():
    assert sorted(c.name for c in cases.all_cases()) == sorted(cases.case_names())
    v = cases.streams()
    for name in ("mixed_4k", "mixed_20k", "mixed_64k"):
        _, chunks, total = cases.chain(v[name][0])
        assert 4096 <= total <= 65536 and all(64 <= c.n <= 4096 for c in chunks[:-1]) and {c.kind for c in chunks} == {0, 1}, name
    _, chunks, _ = cases.chain(v["both_types_65536"][0])
    assert {(c.kind, c.n) for c in chunks} >= {(0, 65536), (1, 65536)}
    want = {c.name: cases.expected(c) for c in cases.all_cases()}
    idx, rs = want["batch_and_malformed"]
    assert idx.count(cases.INVALID) == 1 and {w[0] for w in rs} == {cases.OK, cases.OUT_OF_BOUNDS}
    assert {w[0] for w in want["damage"][1]} == {cases.OK, cases.INVALID, cases.CRC_MISMATCH}
    assert {w[0] for w in want["damage_no_verify"][1]} == {cases.OK, cases.INVALID}
    # two_bad_chunks: the range over both names the lower one, the range over the later alone names that one
    c = cases.case("damage")
    i = [label for label, _ in c.streams].index("two_bad_chunks")
    named = [w[1] for r, w in zip(c.ranges, want["damage"][1]) if r[0] == i and w[0] != cases.OK]
    assert len(set(named)) == 2 and min(named) == named[2], named
    for name in cases.case_names():
        if name.startswith("edges_") and name != "edges_identifier_alone":
            assert all(w[0] == cases.OK for w in want[name][1]) and any(len(w[2]) > 1 for w in want[name][1]), name
    label, s, k, rs = cases.stale_case()
    _, chunks, _ = cases.chain(s)
    touching = [cases.touched(chunks, off, n)[0] <= k <= cases.touched(chunks, off, n)[1] for off, n in rs]
    assert touching.count(True) >= 3 and touching.count(False) >= 3
