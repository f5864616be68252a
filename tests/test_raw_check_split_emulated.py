"""CPU tests of the split check of raw Snappy streams: the UNMODIFIED kernels of
pim-compression_amd/csrc/snappy_raw_check_split.hpp on the lockstep wave emulator, the five of them in the order
snappy_hip_raw_check_split_batch enqueues them.  Every src ends at an inaccessible page, so a byte read behind a stream is a
fault -- which is why every body below runs in a child process that names the step it is on.  (status, out_len) must be what the
independent decoder (raw_cases.expect) and the emulated serial checker (emu_check_lib.raw_check) give the same items; the four
result words must be the model's (tests/raw_check_split_cases.py): every valid large stream proven by the parallel path,
whatever built it -- which is what the split DECODE cannot do, and what these tests count."""
import os
import random
import subprocess
import sys

import pytest

import emu_check_lib as ec
import emu_raw_check_split_lib as ev
import raw_cases as rc
import raw_check_split_cases as vc
import raw_split_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))


def step(*what):
    print("step", *what, flush=True)


def run(items, segment_bytes, **kw):
    r, c = ev.check_split(items, segment_bytes, **kw)
    assert r == 0, "a kernel wrote behind the scratch (101): %d" % r
    return c


def same_verdicts(items, c):
    """the finished call against raw_cases.expect and the emulated serial checker, item by item"""
    serial = ec.raw_check(items, grid=2)
    for i, it in enumerate(items):
        s, null_src = (it[0], bool(it[1] & 1)) if isinstance(it, tuple) else (it, False)
        want = vc.expected(s, null_src) if not isinstance(it, tuple) or len(it) < 3 else serial[i]     # (a claimed src_len: the serial call alone)
        assert c.verdicts[i] == want == serial[i], (i, c.verdicts[i], want, serial[i])


def check(streams, segment_bytes, max_segments=None, trace=False, **kw):
    """one call over plain streams: verdicts, the model's words and -- traced -- the model's nodes for every valid large item"""
    c = run(streams, segment_bytes, max_segments=max_segments, trace=trace, **kw)
    same_verdicts(streams, c)
    want = vc.batch_words(streams, segment_bytes, max_segments)
    assert c.result == want, (c.result, want)
    if trace:
        for i, s in enumerate(streams):
            large = vc.is_large(s, segment_bytes)
            assert (c.plan_flags[i] & ev.FLAG_CLASS == ev.CLASS_SPLIT) == large, i
            if c.nodes[i] is None:
                assert not large or c.plan_flags[i] & ev.FLAG_FALLBACK, i
            elif c.verdicts[i][0] == rc.OK:
                step("trace of item", i)
                assert not c.step4_flags[i] & ev.FLAG_FALLBACK, i
                assert c.nodes[i] == vc.nodes(s, segment_bytes), (i, [(k, g, w) for k, (g, w) in enumerate(zip(c.nodes[i], vc.nodes(s, segment_bytes))) if g != w][:4])
            else:
                assert c.step4_flags[i] & ev.FLAG_FALLBACK, i
    return c


# ---- third-party streams ----
def body_fixtures(segment_bytes):
    streams = [rc.fixture_stream(name) for name in rc.FIXTURES]
    step("fixtures, segments of", segment_bytes)
    c = check(streams, segment_bytes, trace=segment_bytes <= 1024)
    large = sum(vc.is_large(s, segment_bytes) for s in streams)
    assert c.result == [large, len(streams) - large, 0, 0] and c.verdicts == [(rc.OK, len(rc.fixture_plain(n))) for n in rc.FIXTURES]
    if segment_bytes == 1024:
        # what the split decode makes of the same streams at a unit of 32,768: these four fall back there, and `coding` is small
        names = ("terror2", "plrabn12", "random200000", "zeros300000")
        for name in names:
            m = sc.model(rc.fixture_stream(name), 32768, 1024)
            assert m.split_class and m.words == sc.FELL_BACK, name
        m = sc.model(rc.fixture_stream("random200000"), 32768, 1024)
        assert m.segments == 196 and len(m.nodes) == 4
        assert sc.model(rc.fixture_stream("coding"), 32768, 1024).segments == 7 and not sc.model(rc.fixture_stream("coding"), 32768, 1024).split_class
        assert large == 5                                   # (alice is 267 bytes)
    if segment_bytes == vc.DEFAULT_SEGMENT:
        assert vc.segments(rc.fixture_stream("plrabn12"), segment_bytes) == 20


# ---- any valid stream, and what the split decode makes of it ----
DECODE_FALLS_BACK = ((56, 108), (43, 101), (50, 89))        # of the valid large items of sc.model_batch, per config


def body_model_batch(k):
    config = sc.CONFIGS[k]
    batch = sc.model_batch(config)
    streams = [s for _, s, _ in batch]
    models = [sc.model(s, *config) for s in streams]
    decode_large = [m for m in models if m.valid and m.split_class]
    assert (sum(m.words == sc.FELL_BACK for m in decode_large), len(decode_large)) == DECODE_FALLS_BACK[k]
    step("model batch", config, "of", len(streams))
    c = check(streams, config[1], trace=True)
    for i, m in enumerate(models):                          # every item the decode calls large is large here, and proven
        if m.valid and m.split_class:
            assert vc.words(streams[i], config[1]) == vc.SPLIT and not c.step4_flags[i] & ev.FLAG_FALLBACK, i
    assert c.result[0] >= len(decode_large) and c.result[2] == 0, c.result


def body_stream_ends():
    ends = sc.stream_ends()
    streams = [s for pair in ends.values() for s in pair] + list(sc.hostile_ends().values()) + list(sc.copy_reach_streams().values())
    step("stream ends")
    c = check(streams, 128, grid=2, trace=True)
    valid = len(ends) + len(sc.copy_reach_streams())
    assert c.result == [valid, 0, len(streams) - valid, 0], c.result


def body_hand_streams():
    hand = vc.hand_streams()
    for name, (s, (st, want)) in hand.items():
        step(name)
        c = check([s], vc.HAND_SEGMENT, grid=2, trace=True)
        assert c.verdicts[0][0] == st and c.result == want, (name, c.verdicts, c.result)
    step("all of them in one call")
    c = check([s for s, _ in hand.values()], vc.HAND_SEGMENT, trace=True)
    assert c.result == [len(hand) // 3, 0, 2 * len(hand) // 3, 0], c.result


def body_mixed_batch():
    items = list(rc.damaged_vectors().values()) + list(rc.intact_vectors().values())
    s = rc.intact_vectors()["all_types"]
    items += [b"", (s, 1), (s, 1, len(s)), (s, 0, len(s) - 1)] + [h[0] for h in vc.hand_streams().values()][:9]
    step("mixed batch of", len(items))
    c = run(items, 128, grid=2)
    same_verdicts(items, c)
    assert sorted(set(v[0] for v in c.verdicts)) == [rc.OK, rc.INVALID]
    want = [0, 0, 0, 0]
    for it in items:
        w = vc.words(it[0][:it[2]], 128, bool(it[1] & 1)) if isinstance(it, tuple) and len(it) > 2 else \
            vc.words(it[0], 128, True) if isinstance(it, tuple) else vc.words(it, 128)
        want = [a + b for a, b in zip(want, w)]
    assert c.result == want and all(c.result[:3]), (c.result, want)


def body_planner_trips():
    streams = [s for s, _ in sc.planner_trip_items()]
    for max_segments in vc.planner_trip_limits(streams, 128):
        step("planner trips, limit", max_segments)
        c = check(streams, 128, max_segments=max_segments, trace=True)
        fits = max_segments is None or max_segments == vc.planner_trip_limits(streams, 128)[-1]
        assert c.result == [4 if fits else 3, sc.TRIP_COUNT - 4, 0 if fits else 1, 0], c.result
    step("no room at all")
    c = check(streams, 128, max_segments=0)
    assert c.result == [0, sc.TRIP_COUNT - 4, 4, 0]
    step("no items")
    r, c = ev.check_split([], 128, max_segments=4, grid=1)
    assert r == 0 and c.result == [0, 0, 0, 0]


def body_damaged_rich_streams():
    damaged = sc.damaged_rich_streams()
    streams = [s for s, _ in damaged]
    assert len(streams) == 600 and max(len(s) for s in streams) == 16352
    step("600 damaged rich streams")
    c = check(streams, 128, trace=True)
    ok = sum(v[0] == rc.OK for v in c.verdicts)
    assert ok == 314 and c.result[0] > 0 and c.result[2] > 0 and c.result[0] + c.result[1] >= ok, (ok, c.result)


def body_flipped_bytes():
    s = rc.fixture_stream("plrabn12")
    rnd = random.Random(20240607)
    streams = []
    for _ in range(5):
        at = rnd.randrange(3, len(s))
        streams.append(s[:at] + bytes([s[at] ^ (1 << rnd.randrange(8))]) + s[at + 1:])
    step("five flipped bytes")
    check(streams, 4096)


BODIES = {f.__name__[5:]: f for f in (body_fixtures, body_model_batch, body_stream_ends, body_hand_streams, body_mixed_batch, body_planner_trips,
                                      body_damaged_rich_streams, body_flipped_bytes)}


def in_child(name, *args):
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import conftest, test_raw_check_split_emulated as t\n"
            "t.BODIES[sys.argv[2]](*[int(a) for a in sys.argv[3:]])\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code, HERE, name] + [str(a) for a in args], capture_output=True, text=True, timeout=1500)
    lines = out.stdout.strip().splitlines()
    last = next((ln for ln in reversed(lines) if ln.startswith("step ")), "none")
    assert out.returncode == 0 and lines and lines[-1] == "ok", \
        ("status %d (negative: a signal, i.e. an access outside a guarded buffer) at %s" % (out.returncode, last), out.stderr[-2000:])


@pytest.mark.parametrize("segment_bytes", [128, 1024, 4096, vc.DEFAULT_SEGMENT])
def test_third_party_fixtures_are_proven_whatever_the_segment(segment_bytes):
    """The six pyarrow streams in one batch: every one with more than one segment is proven by the parallel path.  At 1,024
    bytes that is all but the 267 bytes of `alice` -- among them the four the split decode hands to the serial decoder at a unit of 32,768, random200000
    with 196 segments and 4 nodes, and `coding`, which is small for the decode.  At the default plrabn12 has 20 segments."""
    in_child("fixtures", segment_bytes)


@pytest.mark.parametrize("k", range(len(sc.CONFIGS)))
def test_any_valid_large_stream_is_proven_where_the_decode_falls_back(k):
    """About a hundred valid items per call (raw_split_cases.model_batch).  The split decode falls back on 56 of 108, 43 of 101
    and 50 of 89 of the large ones; here every one is in word [0], none in word [2], and the nodes after step 3 are the model's."""
    in_child("model_batch", k)


def test_stream_ends_hostile_ends_and_copies_at_a_units_edge():
    in_child("stream_ends")


def test_copies_at_their_absolute_position_in_every_node_and_window():
    """copy_1, copy_2 and copy_4 in the first, a middle and the last node, in the node's first window and deeper: an offset equal
    to the absolute output position is proven, one byte more and an offset of 0 are INVALID through the serial checker."""
    in_child("hand_streams")


def test_mixed_batch_equals_the_serial_check_item_by_item():
    in_child("mixed_batch")


def test_more_items_than_one_trip_of_the_planner_and_the_limit():
    in_child("planner_trips")


def test_damaged_rich_streams_get_both_verdicts():
    in_child("damaged_rich_streams")


def test_flipped_bytes_get_the_serial_verdict():
    in_child("flipped_bytes")
