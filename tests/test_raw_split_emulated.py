"""CPU tests of the split decode of raw Snappy streams: the UNMODIFIED kernels of pim-compression_amd/csrc/snappy_raw_split.hpp
on the lockstep wave emulator, the six of them in the order snappy_hip_raw_decompress_split_batch enqueues them.  Every dst is
a window of exactly its capacity between inaccessible pages and every src ends at one, so a byte written outside a window or
read behind a stream is a fault -- which is why every body below runs in a child process that names the step it is on.  The
oracle is the plaintext; status and length must be what the serial kernel (emu_raw_lib.decompress) gives the same items.
A mistake in steps 2-4 costs fallbacks, never a byte, so the result words, the cuts and the nodes are held to a model of those
steps in plain Python (tests/raw_split_cases.py), on streams of elements that no greedy compressor writes."""
import os
import random
import subprocess
import sys

import pytest

import datagen
import emu_raw_lib as er
import emu_raw_split_lib as es
import raw_cases as rc
import raw_split_cases as sc
from conftest import golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = bytes([rc.GUARD])


def step(*what):
    print("step", *what, flush=True)


def same_as_serial(items, b, plains=None):
    """the finished split batch b against the serial kernel on the same items (and the plaintexts, where given)"""
    r, want = er.decompress(items, grid=2)
    assert r == 0
    for i, it in enumerate(items):
        step("item", i)
        got = (int(b.status[i]), int(b.out_len[i]))
        assert got == (int(want.status[i]), int(want.out_len[i])), (i, got, int(want.status[i]), int(want.out_len[i]))
        n, cap = got[1], int(it[1])
        w, ww = b.window(i), want.window(i)
        if got[0] == rc.OK:
            assert w == ww, (i, next(k for k in range(cap) if w[k] != ww[k]))
            if plains is not None:
                assert w[:n] == plains[i], i
        if ww == FILL * cap:
            assert w == FILL * cap, i                 # untouched where the serial call leaves it untouched
        assert w[min(n, cap):] == FILL * (cap - min(n, cap)), i
    return want


def run(items, unit_len, segment_bytes, **kw):
    r, b = es.decompress_split(items, unit_len, segment_bytes, **kw)
    assert r == 0, "a kernel wrote in front of a window (100) or behind the scratch (101): %d" % r
    return b


def result(b):
    return [int(x) for x in b.result[:4]]


# ---- third-party streams ----
def body_fixtures(segment_bytes):
    plains = [rc.fixture_plain(name) for name in rc.FIXTURES]
    items = [(rc.fixture_stream(name), len(p)) for name, p in zip(rc.FIXTURES, plains)]
    large = sum(len(p) > 65536 for p in plains)
    step("fixtures, segments of", segment_bytes)
    b = run(items, 65536, segment_bytes)
    # every cut exists and no copy crosses a multiple of 65,536 in these streams: a fallback is a bug
    assert result(b) == [large, len(items) - large, 0, 0] and large == 4, result(b)
    for i, p in enumerate(plains):
        assert int(b.status[i]) == rc.OK and b.window(i) == p, rc.FIXTURES[i]
    if segment_bytes == 128:
        same_as_serial(items, b, plains)


def body_fixtures_fall_back():
    """at 32,768 plrabn12 lacks 4 boundaries and has copies across the others, terror2 lacks 2 boundaries"""
    names = ["plrabn12", "terror2"]
    plains = [rc.fixture_plain(n) for n in names]
    items = [(rc.fixture_stream(n), len(p)) for n, p in zip(names, plains)]
    step("unit_len 32768")
    b = run(items, 32768, 1024)
    assert result(b) == [0, 0, 2, 0], result(b)
    same_as_serial(items, b, plains)


# ---- our own compressor ----
def body_own_compressor():
    text = golden_bytes("plrabn12.txt")
    plains = [datagen.text_random_interleave(text, 5000), datagen.text_random_interleave(text, 70001, seed=9)]
    step("compress")
    r, c = er.compress([(p, len(p) + len(p) // 6 + 64 * (len(p) // 1024 + 2)) for p in plains], 1024, 80, grid=3)
    assert r == 0 and [int(x) for x in c.status[:2]] == [rc.OK, rc.OK]
    streams = [c.window(i)[:int(c.out_len[i])] for i in range(2)]
    items = [(s, len(p)) for s, p in zip(streams, plains)]
    for unit_len in (1024, 2048):
        step("unit_len", unit_len)
        b = run(items, unit_len, 128)
        assert result(b) == [2, 0, 0, 0], result(b)
        for i, p in enumerate(plains):
            assert int(b.status[i]) == rc.OK and int(b.out_len[i]) == len(p) and b.window(i) == p, i


# ---- hand-built streams (unit_len 256, segments of 128 bytes) ----
def literals(sizes, seed):
    data = datagen.random_bytes(sum(sizes), seed=seed)
    out, at = [], 0
    for n in sizes:
        out.append(rc.literal(data[at:at + n]))
        at += n
    return out


def hand_streams():
    """name -> (stream, result words expected).  Headers are 2 bytes, so segments start at 2 + 128 k."""
    r = datagen.random_bytes
    unit = [60, 60, 60, 60, 16]                       # a unit of 256 output bytes in literals
    v = {}
    # a copy at a unit's start that reaches into the unit before it: the unit is refused, the serial decoder takes the item
    v["copy2_into_previous_unit"] = (rc._sized(literals(unit, 1) + [rc.copy2(10, 20)] + literals([60, 60, 60, 60, 6] + unit, 2)), [0, 0, 1, 0])
    # no element starts at output byte 256
    v["literal_across_unit_boundary"] = (rc._sized([rc.literal(r(300, seed=3)), rc.literal(r(300, seed=4))]), [0, 0, 1, 0])
    # a COPY_4 inside its unit
    v["copy4_inside_unit"] = (rc._sized(literals(unit, 5) + [rc.literal(r(100, seed=6)), rc.copy4(64, 50), rc.literal(r(92, seed=7))] + literals(unit, 8)),
                              [1, 0, 0, 0])
    # the third element ends exactly on the first segment boundary (60 + 60 + 8 = 128 compressed bytes), one byte behind it, and
    # -- a 61-byte literal that starts one byte in front of the boundary -- 60 bytes behind it
    v["element_ends_on_segment_boundary"] = (rc._sized(literals([59, 59, 7, 60, 60, 11] + unit * 3, 9)), [1, 0, 0, 0])
    v["element_overshoots_by_1"] = (rc._sized(literals([59, 59, 8, 60, 60, 10] + unit * 3, 10)), [1, 0, 0, 0])
    v["element_overshoots_by_60"] = (rc._sized(literals([59, 59, 6, 60, 60, 12] + unit * 3, 11)), [1, 0, 0, 0])
    # a literal as long as a unit, over two segment starts: the element behind it starts 66 bytes into its segment, behind
    # the zone (320 + 258 = 4 * 128 + 66), so the resolve step walks to the segment's end itself
    v["entry_behind_the_zone"] = (rc._sized(literals(unit, 12) + [rc.literal(r(256, seed=13))] + literals(unit + [7], 14)), [1, 0, 0, 0])
    return v


def body_hand_streams():
    for name, (s, want) in hand_streams().items():
        n = rc.header_parses(s)[0]
        assert rc.header_parses(s)[1] == 2 and rc.expect(s)[0] == rc.OK, name
        step(name)
        items = [(s, n + 5)]
        b = run(items, 256, 128, grid=2)
        assert result(b) == want, (name, result(b))
        same_as_serial(items, b, [rc.expect(s)[2]])
    assert len(rc.literal(b"x" * 59)) == 60 and len(rc.literal(b"x" * 60)) == 61 and len(rc.literal(b"x" * 256)) == 258   # (the layouts above)


# ---- one mixed batch ----
def mixed_items():
    items = []
    for s in list(rc.damaged_vectors().values()) + list(rc.intact_vectors().values()):
        h = rc.header_parses(s)
        items.append((s, h[0] if h and h[0] < (1 << 22) else 64))
    s = rc.intact_vectors()["all_types"]
    n = rc.header_parses(s)[0]
    items += [(b"", 16), (s, n, 1), (s, 0), (s, n - 1), (s, n, 2), (rc.fixture_stream("coding"), 9423 - 1), (rc.fixture_stream("coding"), 9423 + 7)]
    items += [(h[0], rc.header_parses(h[0])[0] + 3) for h in hand_streams().values()]
    return items


def body_mixed_batch():
    items = mixed_items()
    step("mixed batch of", len(items))
    b = run(items, 256, 128, grid=2)
    want = same_as_serial(items, b)
    assert sorted(set(int(x) for x in want.status[:len(items)])) == [rc.OK, rc.INVALID, rc.DST_TOO_SMALL]
    res = result(b)
    assert res[0] > 0 and res[1] > 0 and res[2] > 0 and res[3] == 0 and sum(res) <= len(items), res


# ---- damage ----
def body_flipped_bytes():
    s = rc.fixture_stream("plrabn12")
    n = len(rc.fixture_plain("plrabn12"))
    rnd = random.Random(20240607)
    items = []
    for _ in range(5):
        at = rnd.randrange(3, len(s))
        items.append((s[:at] + bytes([s[at] ^ (1 << rnd.randrange(8))]) + s[at + 1:], n))
    step("five flipped bytes")
    b = run(items, 65536, 4096)
    same_as_serial(items, b)


# ---- limits ----
def body_limits():
    names = ["terror2", "plrabn12", "coding"]
    plains = [rc.fixture_plain(n) for n in names]
    items = [(rc.fixture_stream(n), len(p)) for n, p in zip(names, plains)]
    for kw in ({"max_units": 3}, {"max_segments": 10}, {"max_units": 0}, {"max_segments": 1}):
        step("limits", kw)
        b = run(items, 65536, 8192, **kw)
        first = 1 if kw.get("max_units") == 3 or kw.get("max_segments") == 10 else 0       # terror2: 2 units, 7 segments
        assert result(b) == [first, 1, 2 - first, 0], (kw, result(b))
        for i, p in enumerate(plains):
            assert int(b.status[i]) == rc.OK and int(b.out_len[i]) == len(p) and b.window(i) == p, (kw, i)
    assert (len(items[0][0]) - 3 + 8191) // 8192 <= 10 < (len(items[1][0]) - 3 + 8191) // 8192
    step("no items")
    r, b = es.decompress_split([], 65536, 65536, max_segments=4, max_units=4, grid=1)
    assert r == 0 and result(b) == [0, 0, 0, 0]


# ---- steps 2-4 against the model (tests/raw_split_cases.py) ----
def same_as_model(b, models, limits=(None, None)):
    """a traced batch of VALID items against the model: the result words; the plan's classes; no mark from steps 2-4; for every
    split-class item inside the limits its cuts in every slot (NONE where no element starts, src_len at the end) and its nodes"""
    assert result(b) == sc.batch_words(models, *limits), (result(b), sc.batch_words(models, *limits))
    traced = 0
    for i, m in enumerate(models):
        step("trace of item", i)
        assert m.valid and (b.plan_flags[i] & es.FLAG_CLASS == es.CLASS_SPLIT) == m.split_class and b.plan_flags[i] >> 8 == m.hdr, i
        if b.cuts[i] is None:
            assert not m.split_class or b.plan_flags[i] & es.FLAG_FALLBACK, i
            continue
        traced += 1
        assert not b.step4_flags[i] & es.FLAG_FALLBACK, i
        assert b.cuts[i] == m.cuts, (i, [(k, c, w) for k, (c, w) in enumerate(zip(b.cuts[i], m.cuts)) if c != w][:4])
        want = [m.nodes.get(s) for s in range(m.segments)]
        assert b.nodes[i] == want, (i, [(s, g, w) for s, (g, w) in enumerate(zip(b.nodes[i], want)) if g != w][:4])
    return traced


def body_fragment_built():
    for unit_len, segment_bytes, items in sc.fragment_built_calls():
        step("fragment-built, units of", unit_len, "segments of", segment_bytes)
        b = run([(s, len(p)) for s, p in items], unit_len, segment_bytes, trace=True)
        assert result(b) == [len(items), 0, 0, 0], result(b)
        for i, (s, p) in enumerate(items):
            assert (int(b.status[i]), int(b.out_len[i])) == (rc.OK, len(p)) and b.window(i) == p, i
        assert same_as_model(b, [sc.model(s, unit_len, segment_bytes) for s, _ in items]) == len(items)


def body_model_batch(k):
    config = sc.CONFIGS[k]
    batch = sc.model_batch(config)
    models = [sc.model(s, *config) for _, s, _ in batch]
    sc.assert_covers(models)
    items = [(s, len(p) + i % 3) for i, (_, s, p) in enumerate(batch)]
    step("model batch", config, "of", len(items))
    b = run(items, *config, trace=True)
    same_as_model(b, models)
    same_as_serial(items, b, [p for _, _, p in batch])


def body_stream_ends():
    ends = sc.stream_ends()
    streams = [s for pair in ends.values() for s in pair] + list(sc.hostile_ends().values())
    models = [sc.model(s, 256, 128) for s in streams]
    items = [(s, 768) for s in streams]
    step("stream ends")
    b = run(items, 256, 128, grid=2, trace=True)
    valid = [m for m in models if m.valid]
    assert len(valid) == len(ends) and result(b) == [len(valid), 0, len(streams) - len(valid), 0], result(b)
    want = same_as_serial(items, b)
    for i, (s, m) in enumerate(zip(streams, models)):
        step("end", i)
        st, n, plain = rc.expect(s)
        assert (int(want.status[i]), int(want.out_len[i])) == (st, n) and (st == rc.OK) == m.valid, i
        assert m.split_class and m.entry_offsets[m.segments - 2] < sc.ZONE           # (the last segment's lanes and a lookup end on it)
        assert b.nodes[i] == [m.nodes.get(k) for k in range(m.segments)], (i, b.nodes[i])
        if m.valid:
            assert b.window(i) == plain and b.cuts[i] == m.cuts and not b.step4_flags[i] & es.FLAG_FALLBACK, i
        else:                                             # no chain: step 3 marks it, no cut is ever written
            assert b.step4_flags[i] & es.FLAG_FALLBACK and b.cuts[i] == [sc.NONE] * 4, (i, b.cuts[i])


def body_planner_trips():
    batch = sc.planner_trip_items()
    models = [sc.model(s, 256, 128) for s, _ in batch]
    items = [(s, len(p)) for s, p in batch]
    for max_segments, max_units in sc.planner_trip_limits(models):
        step("planner trips, limits", max_segments, max_units)
        b = run(items, 256, 128, max_segments=max_segments, max_units=max_units, trace=True)
        inside = same_as_model(b, models, (max_segments, max_units))
        assert inside == (4 if sc.batch_words(models, max_segments, max_units) == sc.batch_words(models) else 3)
        for i, (s, p) in enumerate(batch):
            assert (int(b.status[i]), int(b.out_len[i])) == (rc.OK, len(p)) and b.window(i) == p, i


BODIES = {f.__name__[5:]: f for f in (body_fixtures, body_fixtures_fall_back, body_own_compressor, body_hand_streams, body_mixed_batch,
                                      body_flipped_bytes, body_limits, body_fragment_built, body_model_batch, body_stream_ends,
                                      body_planner_trips)}


def in_child(name, *args):
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import conftest, test_raw_split_emulated as t\n"
            "t.BODIES[sys.argv[2]](*[int(a) for a in sys.argv[3:]])\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code, HERE, name] + [str(a) for a in args], capture_output=True, text=True, timeout=1500)
    lines = out.stdout.strip().splitlines()
    last = next((ln for ln in reversed(lines) if ln.startswith("step ")), "none")
    assert out.returncode == 0 and lines and lines[-1] == "ok", \
        ("status %d (negative: a signal, i.e. an access outside a guarded buffer) at %s" % (out.returncode, last), out.stderr[-2000:])


@pytest.mark.parametrize("segment_bytes", [128, 1024, 4096])
def test_third_party_fixtures_split_without_a_fallback(segment_bytes):
    """The six pyarrow streams in one batch at unit_len 65,536: the four above 64 KiB go the split path and none falls back;
    random200000 has literals over hundreds of segments (resolve's walked entries), zeros300000 chains of 64-byte copies."""
    in_child("fixtures", segment_bytes)


def test_fixtures_without_independent_units_fall_back_and_decode():
    in_child("fixtures_fall_back")


def test_streams_of_the_own_compressor_split_at_their_block_size_and_its_double():
    in_child("own_compressor")


def test_hand_built_streams():
    """A copy into the previous unit and a literal across a unit boundary (fallback, right bytes); a COPY_4; elements that end on
    a segment boundary, one byte and 60 bytes behind it; a literal over several segments."""
    in_child("hand_streams")


def test_mixed_batch_equals_the_serial_call_item_by_item():
    in_child("mixed_batch")


def test_flipped_bytes_get_the_serial_verdict():
    in_child("flipped_bytes")


def test_items_beyond_the_limits_fall_back_and_the_others_complete():
    in_child("limits")


def test_fragment_built_streams_never_fall_back():
    """Streams of elements no greedy compressor writes, fragment-built by construction: every flavour, units of the fragment and
    of twice the fragment, padded headers: exactly [n, 0, 0, 0], the plaintext, and the model's cuts and nodes."""
    in_child("fragment_built")


@pytest.mark.parametrize("k", range(len(sc.CONFIGS)))
def test_any_valid_stream_gets_the_models_words_cuts_and_nodes(k):
    """About a hundred valid items in one call -- fragment-built at units that fit and that do not, raw-only elements, the hand
    streams, the stream ends, the fixtures (first call): the result words are the model's sums; every cut and every node of
    every split-class item is the model's; status, length and bytes are decode_raw's and the serial call's.  The model's own
    coverage conditions (raw_split_cases.assert_covers) hold for each call."""
    in_child("model_batch", k)


def test_stream_ends_sized_byte_by_byte():
    """Every element kind as the last element, its tag 1-7 bytes in front of src_len: valid, cut short by one byte, and with a
    length field only its fifth byte makes too long."""
    in_child("stream_ends")


def test_more_items_than_one_trip_of_the_planner():
    """1,032 items, split-class ones at 3, 1023, 1024 and 1030; with room for everything and with max_units / max_segments
    ending just in front of and just behind item 1030."""
    in_child("planner_trips")
