"""GPU tests (-m gpu) of snappy_hip_raw_decompress_split_batch through the C ABI and the binding: the fixture, own-compressor,
hand-built, mixed-batch, damage and limit cases of tests/test_raw_split_emulated.py on the device, with guard bytes around
every dst, under the default grid and under SNAPPY_HIP_K2_WAVES=3 (three wavefronts for every persistent kernel); the
drop-in call and one CLI round trip with -S.  The fixtures (at most 482 KB) with segments of 128 to 4,096 bytes are the
smallest shapes with many segments, several units and every case of the resolve step.  All comparisons are exact: the
plaintext, and the serial call (snappy_hip_raw_decompress_batch) on the same items.  The result words of the model-driven
tests come from tests/raw_split_cases.model, never from the device."""
import random

import pytest

import datagen
import emu_raw_split_lib as es
import raw_cases as rc
import raw_split_cases as sc
import test_raw_split_emulated as cases
from conftest import golden_bytes
from test_gpu_raw import FILL, Batch, gpu_compress, gpu_decompress, shb, _cli   # noqa: F401  (shb: the module's fixture)

pytestmark = pytest.mark.gpu
ERR_ARG = 2


def gpu_split(shb, items, unit_len, segment_bytes, max_segments=None, max_units=None):
    import torch
    b = Batch(items)
    b.d_result = torch.full((5,), 0x77, dtype=torch.int32, device="cuda")
    need_s, need_u = es.limits(items, unit_len or 65536, segment_bytes or 16384)
    shb.raw_decompress_split_batch(shb.make_raw_items(b.entries), b.n, unit_len, segment_bytes, need_s if max_segments is None else max_segments,
                                   need_u if max_units is None else max_units, b.d_out_len, b.d_status, b.d_result)
    b.fetch()
    assert b.result[4] == 0x77
    b.result = b.result[:4]
    return b


def same_as_serial(shb, items, b, plains=None):
    want = gpu_decompress(shb, items)
    for i, it in enumerate(items):
        got = (b.status[i], b.out_len[i])
        assert got == (want.status[i], want.out_len[i]), (i, got, want.status[i], want.out_len[i])
        n, cap = got[1], int(it[1])
        w, ww = b.window(i), want.window(i)
        if got[0] == rc.OK:
            assert w == ww, i
            if plains is not None:
                assert w[:n] == plains[i], i
        if ww == FILL * cap:
            assert w == FILL * cap, i                 # untouched where the serial call leaves it untouched
        assert w[min(n, cap):] == FILL * (cap - min(n, cap)), i
    return want


@pytest.fixture(params=[None, "3"], ids=["default_grid", "three_wavefronts"])
def grid(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("SNAPPY_HIP_K2_WAVES", request.param)
    return request.param


@pytest.mark.parametrize("segment_bytes", [128, 1024, 4096])
def test_gpu_split_fixtures_without_a_fallback(shb, grid, segment_bytes):
    plains = [rc.fixture_plain(name) for name in rc.FIXTURES]
    items = [(rc.fixture_stream(name), len(p) + k) for k, (name, p) in enumerate(zip(rc.FIXTURES, plains))]
    b = gpu_split(shb, items, 65536, segment_bytes)
    assert b.result == [4, 2, 0, 0], b.result
    for i, p in enumerate(plains):
        assert (b.status[i], b.out_len[i]) == (rc.OK, len(p)) and b.window(i) == p + FILL * i, rc.FIXTURES[i]
    same_as_serial(shb, items, b)


def test_gpu_split_defaults(shb):
    """the defaults (units of 65,536, segments of 16,384): plrabn12, and a fragment-built stream of elements no greedy compressor
    writes, 5 units and 17 segments long"""
    plain = rc.fixture_plain("plrabn12")
    s, p = sc.fragment_stream(4 * 65536 + 12345, 65536, 77, 2)
    m = sc.model(s, 65536, 16384)
    assert m.words == sc.SPLIT and m.units == 5 and m.segments > 8 and set(range(8)) <= set(m.nodes)
    b = gpu_split(shb, [(rc.fixture_stream("plrabn12"), len(plain)), (s, len(p))], 0, 0)
    assert b.result == [2, 0, 0, 0] and b.status[:2] == [rc.OK, rc.OK] and b.window(0) == plain and b.window(1) == p


def test_gpu_split_fragment_built_streams_never_fall_back(shb, grid):
    """tests/raw_split_cases.fragment_built_calls: exactly [n, 0, 0, 0] and the plaintext"""
    for unit_len, segment_bytes, items in sc.fragment_built_calls():
        b = gpu_split(shb, [(s, len(p)) for s, p in items], unit_len, segment_bytes)
        assert b.result == [len(items), 0, 0, 0], (unit_len, segment_bytes, b.result)
        for i, (s, p) in enumerate(items):
            assert (b.status[i], b.out_len[i]) == (rc.OK, len(p)) and b.window(i) == p, (unit_len, i)


@pytest.fixture(scope="module")
def model_batches():
    """computed once for both grids: [(config, items, plaintexts, the model's result words)]"""
    out = []
    for config in sc.CONFIGS:
        batch = sc.model_batch(config)
        models = [sc.model(s, *config) for _, s, _ in batch]
        sc.assert_covers(models)
        out.append((config, [(s, len(p) + i % 3) for i, (_, s, p) in enumerate(batch)], [p for _, _, p in batch], sc.batch_words(models)))
    return out


@pytest.mark.parametrize("k", range(len(sc.CONFIGS)))
def test_gpu_split_any_valid_stream_gets_the_models_words(shb, grid, model_batches, k):
    """About a hundred valid items in one call; the result words are those of the model of steps 2-4 (a wrong walk, resolve or
    cut shows here and nowhere else); status, length and bytes are decode_raw's and the serial call's."""
    config, items, plains, words = model_batches[k]
    b = gpu_split(shb, items, *config)
    assert b.result == words, (b.result, words)
    same_as_serial(shb, items, b, plains)


def test_gpu_split_stream_ends(shb, grid):
    ends = sc.stream_ends()
    streams = [s for pair in ends.values() for s in pair] + list(sc.hostile_ends().values())
    items = [(s, 768) for s in streams]
    b = gpu_split(shb, items, 256, 128)
    assert b.result == [len(ends), 0, len(streams) - len(ends), 0], b.result
    same_as_serial(shb, items, b)
    for i, s in enumerate(streams):
        st, n, plain = rc.expect(s)
        assert (b.status[i], b.out_len[i]) == (st, n) and (st != rc.OK or b.window(i) == plain), i
    assert [rc.expect(s)[0] for s in streams].count(rc.OK) == len(ends)


def test_gpu_split_more_items_than_one_trip_of_the_planner(shb, grid):
    batch = sc.planner_trip_items()
    models = [sc.model(s, 256, 128) for s, _ in batch]
    items = [(s, len(p)) for s, p in batch]
    for max_segments, max_units in sc.planner_trip_limits(models):
        b = gpu_split(shb, items, 256, 128, max_segments=max_segments, max_units=max_units)
        assert b.result == sc.batch_words(models, max_segments, max_units), (max_segments, max_units, b.result)
        for i, (s, p) in enumerate(batch):
            assert (b.status[i], b.out_len[i]) == (rc.OK, len(p)) and b.window(i) == p, (max_segments, max_units, i)


def test_gpu_split_fixtures_without_independent_units_fall_back(shb, grid):
    names = ["plrabn12", "terror2"]
    plains = [rc.fixture_plain(n) for n in names]
    items = [(rc.fixture_stream(n), len(p)) for n, p in zip(names, plains)]
    b = gpu_split(shb, items, 32768, 1024)
    assert b.result == [0, 0, 2, 0], b.result
    same_as_serial(shb, items, b, plains)


def test_gpu_split_streams_of_the_own_compressor(shb, grid):
    text = golden_bytes("plrabn12.txt")
    plains = [datagen.text_random_interleave(text, 5000), datagen.text_random_interleave(text, 70001, seed=9), datagen.lz_structured(300001, 5)]
    c = gpu_compress(shb, [(p, shb.raw_compress_bound(len(p), 1024)) for p in plains], 1024, 400)
    assert c.status[:3] == [rc.OK] * 3
    items = [(c.window(i)[:c.out_len[i]], len(p)) for i, p in enumerate(plains)]
    for unit_len in (1024, 2048):
        b = gpu_split(shb, items, unit_len, 128)
        assert b.result == [3, 0, 0, 0], (unit_len, b.result)
        for i, p in enumerate(plains):
            assert (b.status[i], b.out_len[i]) == (rc.OK, len(p)) and b.window(i) == p, (unit_len, i)


def test_gpu_split_hand_built_streams(shb, grid):
    for name, (s, want) in cases.hand_streams().items():
        items = [(s, rc.header_parses(s)[0] + 5)]
        b = gpu_split(shb, items, 256, 128)
        assert b.result == want, (name, b.result)
        same_as_serial(shb, items, b, [rc.expect(s)[2]])


def test_gpu_split_mixed_batch_equals_the_serial_call(shb, grid):
    items = cases.mixed_items()
    b = gpu_split(shb, items, 256, 128)
    want = same_as_serial(shb, items, b)
    assert sorted(set(want.status[:b.n])) == [rc.OK, rc.INVALID, rc.DST_TOO_SMALL]
    assert b.result[0] > 0 and b.result[1] > 0 and b.result[2] > 0 and b.result[3] == 0 and sum(b.result) <= len(items), b.result


def test_gpu_split_flipped_bytes_get_the_serial_verdict(shb):
    s = rc.fixture_stream("plrabn12")
    n = len(rc.fixture_plain("plrabn12"))
    rnd = random.Random(20240607)
    items = []
    for _ in range(5):
        at = rnd.randrange(3, len(s))
        items.append((s[:at] + bytes([s[at] ^ (1 << rnd.randrange(8))]) + s[at + 1:], n))
    for segment_bytes in (128, 4096):
        same_as_serial(shb, items, gpu_split(shb, items, 65536, segment_bytes))


def test_gpu_split_damaged_rich_streams_against_the_independent_decoder(shb, grid):
    """the 600 mutations of test_gpu_raw's test through the split call: raw_cases.expect's verdict, decode_raw's bytes"""
    from test_gpu_raw import check_decoded
    items = sc.damaged_rich_streams()
    verdicts = [rc.expect(s, n)[0] for s, n in items]
    b = gpu_split(shb, items, 256, 128)
    for i, (s, n) in enumerate(items):
        check_decoded(b, i, s, n)
    assert b.result[0] > 0 and b.result[2] >= verdicts.count(rc.INVALID) >= 100 and sum(b.result) == len(items), b.result


def test_gpu_split_items_beyond_the_limits_fall_back(shb, grid):
    names = ["terror2", "plrabn12", "coding"]
    plains = [rc.fixture_plain(n) for n in names]
    items = [(rc.fixture_stream(n), len(p)) for n, p in zip(names, plains)]
    for kw in ({"max_units": 3}, {"max_segments": 10}, {"max_units": 0}, {"max_segments": 1}):
        b = gpu_split(shb, items, 65536, 8192, **kw)
        first = 1 if kw.get("max_units") == 3 or kw.get("max_segments") == 10 else 0       # terror2: 2 units, 7 segments
        assert b.result == [first, 1, 2 - first, 0], (kw, b.result)
        for i, p in enumerate(plains):
            assert (b.status[i], b.out_len[i]) == (rc.OK, len(p)) and b.window(i) == p, (kw, i)


def test_gpu_split_arguments(shb):
    import torch
    L = shb.lib()
    assert shb.raw_decompress_split_scratch_bytes(1, 255, 0, 4, 4) == 0 and shb.raw_decompress_split_scratch_bytes(1, 0, 64, 4, 4) == 0
    assert shb.raw_decompress_split_scratch_bytes(1, 0, 192, 4, 4) > 0 and shb.raw_decompress_split_scratch_bytes(1, 0, 200, 4, 4) == 0
    need = shb.raw_decompress_split_scratch_bytes(1, 256, 128, 4, 4)
    assert need == shb.raw_decompress_split_scratch_bytes(1, 0, 0, 4, 4) and need % 256 == 0
    b = Batch([(rc.fixture_stream("coding"), 9423)])
    d_items = shb.make_raw_items(b.entries)
    d_result = torch.full((4,), 0x77, dtype=torch.int32, device="cuda")
    d_scratch = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    at = (-d_scratch.data_ptr()) % 256
    p = d_scratch.data_ptr() + at

    def call(items=d_items.data_ptr(), count=1, unit_len=0, segment_bytes=0, out_len=b.d_out_len.data_ptr(), status=b.d_status.data_ptr(),
             result=d_result.data_ptr(), scratch=p, scratch_bytes=need):
        return L.snappy_hip_raw_decompress_split_batch(items, count, unit_len, segment_bytes, 4, 4, out_len, status, result, scratch, scratch_bytes, None)

    assert call(unit_len=255) == ERR_ARG and call(segment_bytes=64) == ERR_ARG and call(segment_bytes=130) == ERR_ARG
    assert call(items=None) == ERR_ARG and call(out_len=None) == ERR_ARG and call(status=None) == ERR_ARG and call(result=None) == ERR_ARG
    assert call(scratch=None) == ERR_ARG and call(scratch=p + 64) == ERR_ARG and call(scratch_bytes=need - 1) == ERR_ARG
    torch.cuda.synchronize()
    assert d_result.cpu().tolist() == [0x77] * 4                  # a refused call enqueues nothing
    assert call(items=None, count=0, out_len=None, status=None) == 0
    torch.cuda.synchronize()
    assert d_result.cpu().tolist() == [0, 0, 0, 0]                # always written
    assert call() == 0
    b.fetch()
    assert d_result.cpu().tolist() == [0, 1, 0, 0] and b.status[0] == rc.OK and b.window(0) == rc.fixture_plain("coding")


def test_gpu_split_dropin_and_cli_round_trip(shb, tmp_path):
    for name in ("plrabn12", "random200000", "coding"):
        s, plain = rc.fixture_stream(name), rc.fixture_plain(name)
        st, got, rt = shb.raw_decompress_split_host(s)
        assert st == 0 and got == plain, name
        assert set(rt) >= {"pre", "d_alloc", "load", "copy_in", "run", "copy_out", "d_free"}
        assert shb.raw_decompress_split_host(s, 32768)[:2] == (0, plain), name         # (plrabn12: falls back, the same bytes)
    assert shb.raw_decompress_split_host(rc.fixture_stream("coding"), 255)[0] == shb.SNAPPY_INVALID_INPUT
    assert shb.raw_decompress_split_host(rc.damaged_vectors()["offset_0"])[0] == shb.SNAPPY_INVALID_INPUT
    plain = rc.fixture_plain("plrabn12")
    assert shb.raw_decompress_split_host(rc.fixture_stream("plrabn12"), out_capacity=len(plain) - 1)[0] == shb.SNAPPY_BUFFER_TOO_SMALL
    # the CLI: compressed at 4,096-byte fragments, decoded in units of 4,096, of 8,192 and of the default 65,536
    import os
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plrabn12.txt")
    r_c, raw = _cli(["-d", "-c", "-R", "-b", "4096", "-i", src], tmp_path, "plrabn12.raw")
    assert r_c.returncode == 0 and raw, r_c.stderr
    for tag, extra in (("u4096", ["-S", "4096"]), ("u8192", ["-S8192"]), ("default", ["-S"])):
        r_d, got = _cli(["-d", "-R", *extra, "-i", str(tmp_path / "plrabn12.raw")], tmp_path, tag)
        assert r_d.returncode == 0 and got == plain, (tag, r_d.stderr)
    r_h, got = _cli(["-R", "-S", "4096", "-i", str(tmp_path / "plrabn12.raw")], tmp_path, "host")      # host mode ignores -S
    assert r_h.returncode == 0 and got == plain, r_h.stderr
    r_bad, _ = _cli(["-d", "-R", "-S", "100", "-i", str(tmp_path / "plrabn12.raw")], tmp_path, "bad")
    assert r_bad.returncode != 0 and "-S" in r_bad.stderr
