"""GPU tests (-m gpu) of snappy_hip_sz_decompress_split_batch through the C ABI and the binding: the cases of
tests/sz_split_cases.py on the device, one launch per case, with guard bytes around every dst; one 2.5 MiB stream of 32 KiB
chunks at the default segment and at 16 KiB; the one-buffer call; the host-side refusals.  Every answer is compared, exactly, with
snappy_hip_sz_decompress_batch run on the same items in the same test and with the Python model of tests/sz_cases.py;
d_result[2..3] with the cases' model of which large items are proven.  Everything is small: a few MiB in all."""
import pytest

import sz_cases as sz
import sz_split_cases as cases
from test_gpu_raw import Batch
from test_gpu_sz import FILL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return binding


def run(shb, items, max_chunks, segment_bytes, max_segments, flags=0):
    """-> the batch; segment_bytes None: the base call"""
    import torch
    b = Batch(items)
    b.d_bad = torch.full((b.n + 1,), 0x66, dtype=torch.int32, device="cuda")
    b.d_result = torch.full((5,), 0x77, dtype=torch.int32, device="cuda")
    d_items = shb.make_raw_items(b.entries)
    if segment_bytes is None:
        shb.sz_decompress_batch(d_items, b.n, max_chunks, b.d_out_len, b.d_status, b.d_bad, b.d_result, flags=flags)
    else:
        shb.sz_decompress_split_batch(d_items, b.n, max_chunks, segment_bytes, max_segments, b.d_out_len, b.d_status, b.d_bad, b.d_result, flags=flags)
    b.fetch()
    b.bad = [int(x) & 0xffffffff for x in b.d_bad.cpu().numpy()]
    assert b.bad[b.n] == 0x66 and b.result[4] == 0x77
    return b


def check_item(name, b, i, want, capacity):
    st, n, plain, bad = want
    assert (b.status[i], b.out_len[i], b.bad[i]) == (st, n, bad), (name, b.status[i], b.out_len[i], b.bad[i], st, n, bad)
    w = b.window(i)
    if st == sz.OK:
        assert w[:n] == plain and w[n:] == FILL * (capacity - n), name
    elif isinstance(plain, list):                      # a bad chunk: the others are decoded, nothing behind the total is touched
        at = 0
        for piece in plain:
            if piece is None:
                break
            assert w[at:at + len(piece)] == piece, name
            at += len(piece)
        assert w[n:] == FILL * (capacity - n), name
    else:
        assert w == FILL * capacity, name


@pytest.mark.parametrize("name", cases.case_names())
def test_gpu_sz_split_gives_the_base_calls_answers(shb, name):
    c = cases.case(name)
    base = run(shb, c.batch, c.max_chunks, None, 0, flags=c.flags)
    b = run(shb, c.batch, c.max_chunks, c.segment_bytes, c.max_segments, flags=c.flags)
    want, need = cases.expected_items(c)
    for i, it in enumerate(c.items):
        check_item((name, it[0]), b, i, want[i], it[2])
        assert (b.status[i], b.out_len[i], b.bad[i]) == (base.status[i], base.out_len[i], base.bad[i]), (name, it[0])
        assert b.window(i) == base.window(i), (name, it[0])
    assert b.result[:2] == base.result[:2] == [need, sum(w[0] == sz.OK for w in want)]
    assert base.result[2:4] == [0x77, 0x77] and tuple(b.result[2:4]) == cases.expected_split_result(c), b.result


@pytest.fixture(scope="module")
def big():
    plain = sz.text_random_mix(5 * 512 * 1024, 77)
    return sz.write_sz_pyarrow(plain, 32768), plain


@pytest.mark.parametrize("segment_bytes", [0, 16384])
def test_gpu_sz_split_one_stream_of_32_kib_chunks(shb, big, segment_bytes):
    """2.5 MiB of plaintext in chunks of 32,768 bytes, Google's Snappy in the model's frames: at the default segment (1 MiB) and at
    16 KiB, where most shares hold no chunk start at all; in front of it a small item, behind it the same stream cut short."""
    s, plain = big
    assert len(s) > 2 * 1024 * 1024
    small, small_plain = sz.intact_streams()["two_files"]
    items = [(small, len(small_plain)), (s, len(plain) + 5), (s[:-1], len(plain))]
    seg = segment_bytes or 1 << 20
    max_segments = 2 * cases.segments(len(s), seg)
    base = run(shb, items, 200, None, 0)
    b = run(shb, items, 200, segment_bytes, max_segments)
    assert (b.status[:3], b.out_len[:3], b.bad[:3]) == (base.status[:3], base.out_len[:3], base.bad[:3])
    assert b.status[:3] == [sz.OK, sz.OK, sz.INVALID] and b.out_len[:3] == [len(small_plain), len(plain), 0] and b.bad[:3] == [sz.NONE] * 3
    assert b.window(0) == small_plain and b.window(1) == plain + FILL * 5 and b.window(2) == FILL * len(plain)
    assert all(b.window(i) == base.window(i) for i in range(3))
    assert b.result[:4] == [base.result[0], 2, 1, 1] and base.result[0] == 2 + -(-len(plain) // 32768)
    st, n, got, bad = sz.read_sz(s, len(plain) + 5, verify=False)       # (the CRCs are the model writer's own)
    assert (st, n, bad) == (sz.OK, len(plain), sz.NONE) and got == plain
    # a sizing call, then NO_VERIFY over a wrong CRC word in the last chunk
    z = run(shb, [(s, 0, 2), (s, 0)], 200, segment_bytes, max_segments)
    assert z.status[:2] == [sz.DST_TOO_SMALL] * 2 and z.out_len[:2] == [len(plain)] * 2 and z.result[:4] == [0, 0, 2, 0]
    bent = s[:14] + bytes([s[14] ^ 1]) + s[15:]                         # the first chunk's CRC word
    v = run(shb, [(bent, len(plain))], 200, segment_bytes, max_segments)
    assert (v.status[0], v.bad[0]) == (sz.CRC_MISMATCH, 0) and v.result[:4] == [base.result[0] - 2, 0, 1, 0]
    v = run(shb, [(bent, len(plain))], 200, segment_bytes, max_segments, flags=sz.NO_VERIFY)
    assert v.status[0] == sz.OK and v.window(0) == plain


def test_gpu_sz_split_one_buffer_call_round_trips_and_keeps_the_verdicts(shb, big):
    s, plain = big
    st, got, _ = shb.sz_decompress_split_host(s)
    assert st == 0 and got == plain
    mid = sz.text_random_mix(150000, 11)
    st, stream, _ = shb.sz_compress_host(mid, 32768)
    assert st == 0 and shb.sz_decompress_split_host(stream)[:2] == (0, mid)
    assert shb.sz_decompress_split_host(sz.IDENTIFIER)[:2] == (0, b"")
    damaged = sz.damaged_streams()
    for name in ("crc_word_bit_chunk2", "reserved_unskippable_02", "truncated_by_1", "varint_disagrees_longer", "identifier_missing", "elements_damaged"):
        a, b = shb.sz_decompress_split_host(damaged[name]), shb.sz_decompress_host(damaged[name])
        assert a[:2] == b[:2] and a[0] != 0 and a[1] == b"", name
    # a large file damaged behind the first segment: a CRC word in its last chunk
    bent = s[:-40000] + bytes([s[-40000] ^ 0x10]) + s[-39999:]
    a, b = shb.sz_decompress_split_host(bent), shb.sz_decompress_host(bent)
    assert a[:2] == b[:2] and a[0] != 0
    assert shb.sz_decompress_split_host(damaged["crc_word_bit_chunk2"], flags=sz.NO_VERIFY)[0] == 0


def test_gpu_sz_split_host_side_refusals_and_an_empty_batch(shb):
    import torch
    c = cases.case("limit_max_segments")
    for seg in (64, 192, 255, 257, 1000):
        assert shb.sz_decompress_split_scratch_bytes(4, 100, seg, 100) == 0, seg
        with pytest.raises(shb.SnappyHipError):
            run(shb, c.batch, c.max_chunks, seg, 100)
    assert shb.sz_decompress_split_scratch_bytes(4, 100, 0, 100) == shb.sz_decompress_split_scratch_bytes(4, 100, 1 << 20, 100) > \
        shb.sz_decompress_scratch_bytes(4, 100)
    with pytest.raises(shb.SnappyHipError):
        run(shb, c.batch, c.max_chunks, 1024, 100, flags=2)
    b = Batch(c.batch)
    b.d_bad = torch.full((b.n + 1,), 0x66, dtype=torch.int32, device="cuda")
    b.d_result = torch.full((5,), 0x77, dtype=torch.int32, device="cuda")
    d_items = shb.make_raw_items(b.entries)
    need = shb.sz_decompress_split_scratch_bytes(b.n, 100, 1024, 100)
    scratch = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    L, vp = shb.lib(), lambda t: t.data_ptr()
    args = lambda **kw: [kw.get("items", vp(d_items)), b.n, 100, 1024, 100, 0, kw.get("out_len", vp(b.d_out_len)), kw.get("status", vp(b.d_status)),  # noqa: E731
                         kw.get("bad", vp(b.d_bad)), kw.get("result", vp(b.d_result)), kw.get("scratch", vp(scratch)), kw.get("bytes", need), None]
    for bad in ({"items": None}, {"out_len": None}, {"status": None}, {"bad": None}, {"result": None}, {"scratch": None}, {"scratch": vp(scratch) + 64},
                {"bytes": need - 1}):
        assert L.snappy_hip_sz_decompress_split_batch(*args(**bad)) == 2, bad                 # SNAPPY_HIP_ERR_ARG
    torch.cuda.synchronize()
    assert [int(x) for x in b.d_result.cpu().numpy()] == [0x77] * 5 and int(b.d_status.cpu()[0]) == 0x55       # nothing was enqueued
    # count == 0: OK, the four result words written
    shb.sz_decompress_split_batch(d_items, 0, 8, 0, 8, None, None, None, b.d_result)
    torch.cuda.synchronize()
    assert [int(x) for x in b.d_result.cpu().numpy()] == [0, 0, 0, 0, 0x77]
