"""GPU tests (-m gpu) of snappy_hip_raw_check_split_batch through the C ABI and the binding: the groups of
tests/test_raw_check_split_emulated.py on the device, under the default grid and under SNAPPY_HIP_K2_WAVES=3 (three wavefronts
for every persistent kernel); the arguments, the drop-in call and one CLI run each of -d -R -T -S on an intact and a damaged
file.  The fixtures (at most 482 KB) with segments of 128 to 4,096 bytes are the smallest shapes that reach every case of the
walk, the resolve and the verify step.  All comparisons are exact: (status, out_len) with snappy_hip_raw_check_batch on the
same items and with raw_cases.expect, the four result words with the model of tests/raw_check_split_cases.py, never with the
device.  The check reads only: items and streams are byte-identical afterwards and no dst byte is touched."""
import os
import random

import pytest

import raw_cases as rc
import raw_check_split_cases as vc
import raw_split_cases as sc
from test_gpu_raw import Batch, shb   # noqa: F401  (shb: the module's fixture)

pytestmark = pytest.mark.gpu
ERR_ARG = 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _items(entries):
    """plain streams, or (stream, flags) / (stream, flags, src_len) -> what test_gpu_raw.Batch takes, with no room at dst"""
    out = []
    for e in entries:
        e = e if isinstance(e, tuple) else (e,)
        out.append((e[0], 0, e[1] if len(e) > 1 else 0) + ((e[2],) if len(e) > 2 else ()))
    return out


def gpu_check_split(shb, entries, segment_bytes, max_segments=None):
    """-> (the split check's Batch with .result, the serial check's Batch), both fetched; the two agree item by item"""
    import torch
    items = _items(entries)
    b = Batch(items)
    b.d_result = torch.full((5,), 0x77, dtype=torch.int32, device="cuda")
    d_items = shb.make_raw_items([(e[0], e[1], 0, 0) for e in b.entries])          # dst and dst_capacity are ignored: none given
    h_items, h_src = d_items.cpu().numpy().copy(), b.d_src.cpu().numpy().copy()
    need = sum((len(it[0]) + (segment_bytes or vc.DEFAULT_SEGMENT) - 1) // (segment_bytes or vc.DEFAULT_SEGMENT) for it in items)
    shb.raw_check_split_batch(d_items, b.n, segment_bytes, need if max_segments is None else max_segments, b.d_out_len, b.d_status, b.d_result)
    b.fetch()                                                  # (asserts the words behind both arrays and every guard byte)
    assert b.result[4] == 0x77
    b.result = b.result[:4]
    assert (d_items.cpu().numpy() == h_items).all() and (b.d_src.cpu().numpy() == h_src).all() and (b.buf == rc.GUARD).all()
    serial = Batch(items)
    if serial.n:
        shb.raw_check_batch(shb.make_raw_items([(e[0], e[1], 0, 0) for e in serial.entries]), serial.n, serial.d_out_len, serial.d_status)
    serial.fetch()
    for i in range(b.n):
        assert (b.status[i], b.out_len[i]) == (serial.status[i], serial.out_len[i]), (i, b.status[i], b.out_len[i], serial.status[i], serial.out_len[i])
    return b, serial


def check(shb, streams, segment_bytes, max_segments=None):
    """one call over plain streams: the serial check's and raw_cases.expect's verdicts, the model's words"""
    b, _ = gpu_check_split(shb, streams, segment_bytes, max_segments)
    for i, s in enumerate(streams):
        assert (b.status[i], b.out_len[i]) == vc.expected(s), (i, b.status[i], b.out_len[i], vc.expected(s))
    want = vc.batch_words(streams, segment_bytes or vc.DEFAULT_SEGMENT, max_segments)
    assert b.result == want, (b.result, want)
    return b


@pytest.fixture(params=[None, "3"], ids=["default_grid", "three_wavefronts"])
def grid(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("SNAPPY_HIP_K2_WAVES", request.param)
    return request.param


@pytest.mark.parametrize("segment_bytes", [128, 1024, 4096])
def test_gpu_check_split_fixtures_are_proven(shb, grid, segment_bytes):
    """Every fixture of more than one segment is proven: at 1,024 bytes the four that the split decode hands to the serial
    decoder at a unit of 32,768 (random200000 there: 196 segments, 4 nodes), and `coding`, which is small for the decode."""
    streams = [rc.fixture_stream(name) for name in rc.FIXTURES]
    b = check(shb, streams, segment_bytes)
    large = sum(vc.is_large(s, segment_bytes) for s in streams)
    assert b.result == [large, len(streams) - large, 0, 0] and large == (6 if segment_bytes == 128 else 5)
    if segment_bytes == 1024:
        for name in ("terror2", "plrabn12", "random200000", "zeros300000"):
            assert sc.model(rc.fixture_stream(name), 32768, 1024).words == sc.FELL_BACK, name


def test_gpu_check_split_defaults(shb):
    """segment_bytes 0 = 16,384: plrabn12 has 20 segments"""
    streams = [rc.fixture_stream("plrabn12"), rc.fixture_stream("terror2"), rc.fixture_stream("alice")]
    assert vc.segments(streams[0], vc.DEFAULT_SEGMENT) == 20
    b = check(shb, streams, 0)
    assert b.result == [2, 1, 0, 0]


@pytest.fixture(scope="module")
def model_batches():
    """computed once for both grids: [(segment_bytes, streams, valid items the split decode calls large, those it falls back on)]"""
    out = []
    for config in sc.CONFIGS:
        streams = [s for _, s, _ in sc.model_batch(config)]
        large = [m for m in (sc.model(s, *config) for s in streams) if m.valid and m.split_class]
        out.append((config[1], streams, len(large), sum(m.words == sc.FELL_BACK for m in large)))
    return out


@pytest.mark.parametrize("k", range(len(sc.CONFIGS)))
def test_gpu_check_split_any_valid_large_stream_is_proven(shb, grid, model_batches, k):
    """About a hundred valid items per call, of which the split decode falls back on 56 of 108, 43 of 101 and 50 of 89: here every
    large one is in word [0] and none in word [2]."""
    segment_bytes, streams, decode_large, decode_falls_back = model_batches[k]
    assert (decode_falls_back, decode_large) == ((56, 108), (43, 101), (50, 89))[k]
    b = check(shb, streams, segment_bytes)
    assert b.result[0] >= decode_large and b.result[2] == 0 and b.result[0] + b.result[1] == len(streams), b.result


def test_gpu_check_split_stream_ends_and_copy_reach(shb, grid):
    ends = sc.stream_ends()
    streams = [s for pair in ends.values() for s in pair] + list(sc.hostile_ends().values()) + list(sc.copy_reach_streams().values())
    b = check(shb, streams, 128)
    valid = len(ends) + len(sc.copy_reach_streams())
    assert b.result == [valid, 0, len(streams) - valid, 0], b.result


def test_gpu_check_split_copies_at_their_absolute_position(shb, grid):
    """copy_1, copy_2 and copy_4 in the first, a middle and the last node, in the node's first window and deeper: an offset equal
    to the absolute output position is proven; a byte more, or 0, is INVALID through the serial checker.  One call for all, then
    every one alone (a wrong neighbour cannot hide it)."""
    hand = vc.hand_streams()
    b = check(shb, [s for s, _ in hand.values()], vc.HAND_SEGMENT)
    assert b.result == [len(hand) // 3, 0, 2 * len(hand) // 3, 0], b.result
    for i, (name, (s, (st, words))) in enumerate(hand.items()):
        assert b.status[i] == st, name
    for name, (s, (st, words)) in list(hand.items())[::3] + list(hand.items())[1::3]:
        one = check(shb, [s], vc.HAND_SEGMENT)
        assert one.status[0] == st and one.result == words, (name, one.status[0], one.result)


def test_gpu_check_split_more_items_than_one_trip_of_the_planner(shb, grid):
    streams = [s for s, _ in sc.planner_trip_items()]
    limits = vc.planner_trip_limits(streams, 128)
    for max_segments in limits + [0]:
        b = check(shb, streams, 128, max_segments)
        fits = max_segments is None or max_segments == limits[-1]
        want = [0, sc.TRIP_COUNT - 4, 4, 0] if max_segments == 0 else [4 if fits else 3, sc.TRIP_COUNT - 4, 0 if fits else 1, 0]
        assert b.result == want and b.status[:b.n] == [rc.OK] * b.n, (max_segments, b.result)


def test_gpu_check_split_damaged_rich_streams(shb, grid):
    """600 seeded mutations (the longest 16,352 bytes), 314 of them valid: both verdicts, and both of the parallel path's words"""
    streams = [s for s, _ in sc.damaged_rich_streams()]
    b = check(shb, streams, 128)
    assert b.status[:b.n].count(rc.OK) == 314 and b.result[0] > 0 and b.result[2] > 0, b.result


def test_gpu_check_split_flipped_bytes_and_mixed_batch(shb, grid):
    s = rc.fixture_stream("plrabn12")
    rnd = random.Random(20240607)
    streams = []
    for _ in range(5):
        at = rnd.randrange(3, len(s))
        streams.append(s[:at] + bytes([s[at] ^ (1 << rnd.randrange(8))]) + s[at + 1:])
    check(shb, streams, 4096)
    some = rc.intact_vectors()["all_types"]
    big = rc.varint(rc.RAW_MAX_LEN + 1) + rc.literal(b"x")
    entries = list(rc.damaged_vectors().values()) + list(rc.intact_vectors().values()) + \
        [big, b"", (some, 1), (some, 0, rc.RAW_MAX_LEN + 1)]   # a null src; a claimed src_len above the maximum (never read that far)
    b, serial = gpu_check_split(shb, entries, 128)
    assert sorted(set(b.status[:b.n])) == [rc.OK, rc.INVALID, rc.TOO_LARGE]
    plain = [e for e in entries if not isinstance(e, tuple)]
    want = vc.batch_words(plain, 128)                          # (the two last items are settled by their header: in no word)
    assert b.result == want and all(b.result[:3]), (b.result, want)


def test_gpu_check_split_arguments(shb):
    import torch
    lib = shb.lib()
    s = rc.fixture_stream("terror2")
    b = Batch(_items([s]))
    d_items = shb.make_raw_items([(e[0], e[1], 0, 0) for e in b.entries])
    JUNK = 0x77
    d_result = torch.full((4,), JUNK, dtype=torch.int32, device="cuda")
    assert shb.raw_check_split_scratch_bytes(1, 0, 4) == shb.raw_check_split_scratch_bytes(1, 16384, 4) == 256 + 256 + 256 + 4 * 512 + 256
    for bad in (64, 100, 129, 16384 + 32):
        assert shb.raw_check_split_scratch_bytes(1, bad, 4) == 0
    need = shb.raw_check_split_scratch_bytes(1, 1024, 49)
    scratch = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    args = [d_items.data_ptr(), 1, 1024, 49, b.d_out_len.data_ptr(), b.d_status.data_ptr(), d_result.data_ptr(), scratch.data_ptr(), need, None]
    for k, v in ((0, None), (4, None), (5, None), (6, None), (7, None), (7, scratch.data_ptr() + 64), (8, need - 1), (2, 100), (2, 64), (2, 1024 + 32)):
        refused = list(args)
        refused[k] = v
        assert lib.snappy_hip_raw_check_split_batch(*refused) == ERR_ARG, (k, v)
    torch.cuda.synchronize()
    assert (d_result.cpu().numpy() == JUNK).all() and int(b.d_status.cpu()[0]) == 0x55       # a refused call enqueues nothing
    assert lib.snappy_hip_raw_check_split_batch(None, 0, 0, 0, None, None, d_result.data_ptr(), scratch.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in d_result.cpu().numpy()] == [0, 0, 0, 0]
    d_result.fill_(JUNK)
    assert lib.snappy_hip_raw_check_split_batch(*args) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in d_result.cpu().numpy()] == [1, 0, 0, 0] and int(b.d_status.cpu()[0]) == rc.OK and int(b.d_out_len.cpu()[0]) == 105438
    assert vc.segments(s, 1024) == 49


def test_gpu_check_split_dropin_and_cli(shb, tmp_path):
    import subprocess
    from test_cli import CLI, HOST_DIR, run
    for name in rc.FIXTURES:
        s = rc.fixture_stream(name)
        st, n, rt = shb.check_raw_split_host(s)
        assert (st, n) == shb.check_raw_host(s)[:2] == (0, len(rc.fixture_plain(name))) and rt["run"] > 0, name
    s = rc.fixture_stream("plrabn12")
    damaged = bytearray(s)
    damaged[200000] ^= 0x55
    for bad in (s[:len(s) // 2], bytes(damaged), b"", bytes([0x80, 0x80])):
        assert shb.check_raw_split_host(bad)[:2] == shb.check_raw_host(bad)[:2], len(bad)
    assert shb.check_raw_split_host(s[:len(s) // 2])[0] == 1
    subprocess.check_call(["make", "-s", "-C", HOST_DIR])
    raw = os.path.join(GOLDEN, "raw", "plrabn12.raw_snappy")
    r = run(CLI, "-d", "-R", "-T", "-S", "-i", raw)
    assert r.returncode == 0 and "Check: OK, %d bytes\n" % len(rc.fixture_plain("plrabn12")) in r.stdout, (r.stdout, r.stderr)
    cut = tmp_path / "cut.raw_snappy"
    cut.write_bytes(s[:200000])
    r = run(CLI, "-d", "-R", "-T", "-S", "-i", str(cut))
    plain = run(CLI, "-d", "-R", "-T", "-i", str(cut))
    assert r.returncode == plain.returncode == 1 and "Check: INVALID\n" in r.stdout and "Check: INVALID\n" in plain.stdout, (r.stdout, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["cut.raw_snappy"]
