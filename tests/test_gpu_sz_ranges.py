"""GPU tests (-m gpu) of snappy_hip_sz_index_batch and snappy_hip_sz_decompress_ranges through the C ABI and the binding: the
cases of tests/sz_ranges_cases.py on the device with guard bytes around every dst; a stale index; one 2.5 MiB stream of 32 KiB
chunks indexed at the default segment and at 16 KiB with 1,000 seeded ranges, intact, with one CRC word bent, and with a one-slot
scratch; the index against snappy_hip_sz_decompress_split_batch in the same test; the one-buffer calls; the host-side refusals.
Every answer is compared, exactly, with the Python model of tests/sz_ranges_cases.py.  The streams are a few MiB in all; the largest call writes some 30 MiB of ranges."""
import numpy as np
import pytest

import sz_cases as sz
import sz_ranges_cases as cases

pytestmark = pytest.mark.gpu
GAP, GUARD = 64, 0xEE


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return binding


class Index:
    """`streams` (bytes each) in one device buffer, GAP bytes apart, and their index"""

    def __init__(self, shb, streams, max_chunks, segment_bytes=1024, max_segments=512, null_src=()):
        import torch
        self.shb, self.n, self.max_chunks = shb, len(streams), max_chunks
        at, blob = [], bytearray()
        for s in streams:
            blob += bytes(GAP)
            at.append(len(blob))
            blob += s
        self.d_src = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(GAP), dtype=np.uint8).copy()).cuda()
        self.entries = [(0 if i in null_src else self.d_src.data_ptr() + at[i], len(s), 0, 0) for i, s in enumerate(streams)]
        self.d_items = shb.make_raw_items(self.entries)
        self.d_chunks = torch.full((32 * (max_chunks + 1),), 0x3C, dtype=torch.uint8, device="cuda")
        self.d_descs = torch.full((40 * (self.n + 1),), 0x3D, dtype=torch.uint8, device="cuda")
        self.d_status = torch.full((self.n + 1,), 0x55, dtype=torch.int32, device="cuda")
        self.d_result = torch.full((5,), 0x77, dtype=torch.int32, device="cuda")
        shb.sz_index_batch(self.d_items, self.n, max_chunks, segment_bytes, max_segments, self.d_chunks, self.d_descs, self.d_status, self.d_result)
        torch.cuda.synchronize()
        self.status = [int(x) for x in self.d_status.cpu().numpy()]
        self.result = [int(x) & 0xffffffff for x in self.d_result.cpu().numpy()]
        assert self.status[self.n] == 0x55 and self.result[4] == 0x77
        raw = self.d_chunks.cpu().numpy()
        assert (raw[32 * max_chunks:] == 0x3C).all() and (self.d_descs.cpu().numpy()[40 * self.n:] == 0x3D).all()
        self.records = raw[:32 * max_chunks].view(shb.SZ_CHUNK_DTYPE)
        self.descs = self.d_descs.cpu().numpy()[:40 * self.n].view(shb.SZ_DESC_DTYPE)

    def check(self, streams):
        """the statuses, descs and records against the model"""
        models = [cases.index_model(s) for s in streams]
        assert self.status[:self.n] == [m[0] for m in models]
        need = sum(len(m[1]) for m in models)
        assert self.result[:2] == [need, sum(m[0] == cases.OK for m in models)] and need <= self.max_chunks
        at = 0
        for i, (st, recs, total) in enumerate(models):
            d = self.descs[i]
            assert (int(d["src"]), int(d["src_len"]), int(d["num_chunks"]), int(d["total_len"])) == (self.entries[i][0], len(streams[i]), len(recs), total), i
            if recs:
                assert int(d["chunks"]) == self.d_chunks.data_ptr() + 32 * at, i
            got = self.records[at:at + len(recs)]
            assert [tuple(int(x) for x in g) for g in got] == [r[:4] + (i, 0) for r in recs], i
            at += len(recs)

    def ranges(self, ranges, flags=0, slots=None, count=None):
        """ranges: [(stream, offset, length, null_dst)] -> (statuses, bad chunks, windows): every dst between guard bytes"""
        import torch
        shb, m = self.shb, len(ranges)
        lens = np.array([r[2] if r[2] <= 1 << 30 else 0 for r in ranges], dtype=np.int64)
        dst_at = np.cumsum(lens + GAP) - lens
        buf_len = int(dst_at[-1] + lens[-1] + GAP)
        d_dst = torch.full((buf_len,), GUARD, dtype=torch.uint8, device="cuda")
        d_ranges = shb.make_ranges([(r[0], r[1], r[2], 0 if r[3] else d_dst.data_ptr() + int(dst_at[k])) for k, r in enumerate(ranges)])
        d_status = torch.full((m + 1,), 0x55, dtype=torch.int32, device="cuda")
        d_bad = torch.full((m + 1,), 0x66, dtype=torch.int32, device="cuda")
        d_scratch = None
        if slots is not None:       # the parts in front of the slots (what the full grid's size has beyond an empty call's slots), then `slots` slots
            head = shb.sz_decompress_ranges_scratch_bytes(m) - shb.sz_decompress_ranges_scratch_bytes(0) + 256
            d_scratch = torch.empty(head + slots * 65536 + 65535, dtype=torch.uint8, device="cuda")
        shb.sz_decompress_ranges(self.d_descs, self.n if count is None else count, d_ranges, m, d_status, d_bad, flags=flags, d_scratch=d_scratch)
        torch.cuda.synchronize()
        status = [int(x) for x in d_status.cpu().numpy()]
        bad = [int(x) & 0xffffffff for x in d_bad.cpu().numpy()]
        assert status[m] == 0x55 and bad[m] == 0x66
        buf = d_dst.cpu().numpy()
        gaps = (dst_at[:, None] - GAP + np.arange(GAP)[None, :]).ravel()
        assert (buf[gaps] == GUARD).all() and (buf[buf_len - GAP:] == GUARD).all(), "a byte outside every window was written"
        return status[:m], bad[:m], [buf[int(dst_at[k]):int(dst_at[k] + lens[k])].tobytes() for k in range(m)]


def check_ranges(name, got, ranges, want):
    status, bad, windows = got
    for r, (w, q) in enumerate(zip(want, ranges)):
        assert (status[r], bad[r]) == w[:2], (name, r, q[:2], (status[r], bad[r]), w[:2])
        if w[0] == cases.OK:
            assert windows[r] == w[2], (name, r, q[:2])
        elif w[0] == cases.OUT_OF_BOUNDS:
            assert windows[r] == bytes([GUARD]) * len(windows[r]), (name, r, q[:2])


@pytest.mark.parametrize("name", cases.case_names())
def test_gpu_sz_ranges_give_the_models_answers(shb, name):
    c = cases.case(name)
    streams = [s for _, s in c.streams]
    need = sum(len(cases.index_model(s)[1]) for s in streams)
    ix = Index(shb, streams, need + 3)
    ix.check(streams)
    idx, want = cases.expected(c)
    flags = 0 if c.verify else sz.NO_VERIFY
    check_ranges(name, ix.ranges(c.ranges, flags=flags), c.ranges, want)
    check_ranges((name, "one slot"), ix.ranges(c.ranges, flags=flags, slots=1), c.ranges, want)


def test_gpu_sz_ranges_a_stale_record_is_invalid_for_the_ranges_that_touch_it(shb):
    import torch
    label, s, k, rs = cases.stale_case()
    _, chunks, _ = cases.chain(s)
    ranges = [(0, off, n, False) for off, n in rs]
    want = []
    for off, n in rs:
        first, last = cases.touched(chunks, off, n)
        want.append((cases.INVALID, k, None) if first <= k <= last else cases.range_model(s, off, n))
    for name, edit in cases.stale_edits().items():
        ix = Index(shb, [s], len(chunks))
        ix.check([s])
        r = {f: int(ix.records[k][f]) for f in ("src_off", "dst_off", "info", "ulen")}
        edit(r)
        recs = ix.records.copy()
        for f, v in r.items():
            recs[f][k] = v
        ix.d_chunks[:32 * len(chunks)] = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
        check_ranges(("stale", name), ix.ranges(ranges), ranges, want)


@pytest.fixture(scope="module")
def big():
    plain = sz.text_random_mix(5 * 512 * 1024, 77)
    return sz.write_sz_pyarrow(plain, 32768), plain


@pytest.mark.parametrize("segment_bytes", [0, 16384])
def test_gpu_sz_ranges_one_stream_of_32_kib_chunks(shb, big, segment_bytes):
    """2.5 MiB of plaintext in chunks of 32,768 bytes, indexed at the default segment (1 MiB) and at 16 KiB: 1,000 seeded ranges of
    1 to 200,000 bytes against slices of the plaintext; the same ranges after one CRC word is bent -- exactly the ranges the model
    names report CRC_MISMATCH with that chunk; the same ranges with a one-slot scratch.  And the index against
    snappy_hip_sz_decompress_split_batch on the same stream: d_result, the status, total_len == d_out_len."""
    import torch
    s, plain = big
    seg = segment_bytes or 1 << 20
    max_segments = 2 * -(-len(s) // seg)
    chunks_n = -(-len(plain) // 32768)
    ix = Index(shb, [s], chunks_n + 4, segment_bytes, max_segments)
    assert ix.status[0] == cases.OK and ix.result[:4] == [chunks_n, 1, 1, 0]
    assert int(ix.descs[0]["total_len"]) == len(plain) and int(ix.descs[0]["num_chunks"]) == chunks_n
    assert [int(x) for x in ix.records["dst_off"][:chunks_n]] == list(range(0, len(plain), 32768))
    # the split call on the same item
    d_out_len = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_status = torch.full((2,), 0x55, dtype=torch.int32, device="cuda")
    d_bad = torch.full((2,), 0x66, dtype=torch.int32, device="cuda")
    d_result = torch.full((5,), 0x77, dtype=torch.int32, device="cuda")
    d_out = torch.empty(len(plain), dtype=torch.uint8, device="cuda")
    d_items = shb.make_raw_items([(ix.entries[0][0], len(s), d_out.data_ptr(), len(plain))])
    shb.sz_decompress_split_batch(d_items, 1, chunks_n + 4, segment_bytes, max_segments, d_out_len, d_status, d_bad, d_result, flags=sz.NO_VERIFY)
    torch.cuda.synchronize()
    assert [int(x) for x in d_result.cpu().numpy()][:4] == ix.result[:4] and int(d_status[0]) == ix.status[0]
    assert int(d_out_len[0]) == int(ix.descs[0]["total_len"])

    rs = cases.seeded_ranges(len(plain), 1000, 5 + segment_bytes, 200000)
    ranges = [(0, off, n, False) for off, n in rs]
    want = [(cases.OK, cases.NONE, plain[off:off + n]) for off, n in rs]
    check_ranges("intact", ix.ranges(ranges, flags=sz.NO_VERIFY), ranges, want)          # (the CRCs are the model writer's own)
    check_ranges("intact, verified", ix.ranges(ranges), ranges, want)
    check_ranges("one slot", ix.ranges(ranges, slots=1), ranges, want)
    # one CRC word bent: chunk 41's
    k = 41
    at = int(ix.records[k]["src_off"]) + 4
    bent = s[:at] + bytes([s[at] ^ 0x20]) + s[at + 1:]
    bx = Index(shb, [bent], chunks_n + 4, segment_bytes, max_segments)
    want_bent = [(cases.CRC_MISMATCH, k, None) if off // 32768 <= k <= (off + n - 1) // 32768 else w for (off, n), w in zip(rs, want)]
    assert 10 < sum(w[0] != cases.OK for w in want_bent) < 500
    check_ranges("bent", bx.ranges(ranges), ranges, want_bent)
    check_ranges("bent, not verified", bx.ranges(ranges, flags=sz.NO_VERIFY), ranges, want)


def test_gpu_sz_ranges_one_buffer_call_on_intact_and_damaged_files(shb, big):
    """snappy_decompress_sz_range_gpu: a file in host memory, the chain walked on the host up to the range's last chunk"""
    s, plain = big
    for off, n in [(0, 0), (0, 1), (32767, 2), (1000000, 300000), (len(plain) - 1, 1), (len(plain), 0)]:
        st, got, _ = shb.sz_decompress_range_host(s, off, n)
        assert st == 0 and got == plain[off:off + n], (off, n)
    for off, n in [(len(plain), 1), (0, len(plain) + 1), (2 ** 64 - 1, 2)]:
        assert shb.sz_decompress_range_host(s, off, n)[0] != 0, (off, n)
    for name, (s2, p2) in cases.streams().items():
        for off, n in cases.edge_ranges(s2, seed=9, many=2):
            st, got, _ = shb.sz_decompress_range_host(s2, off, n)
            assert st == 0 and got == p2[off:off + n], (name, off, n)
    for name, d in cases.parsing_damage().items():
        for off, n in cases.damage_ranges(d):
            want = cases.range_model(d, off, n)
            st, got, _ = shb.sz_decompress_range_host(d, off, n)
            assert (st == 0) == (want[0] == cases.OK) and (st != 0 or got == want[2]), (name, off, n)
            if want[0] == cases.CRC_MISMATCH:
                assert shb.sz_decompress_range_host(d, off, n, flags=sz.NO_VERIFY)[0] == 0, (name, off, n)
    # a chain broken behind the range is never reached; one broken in front of its end is refused; so is an unknown flag
    cut = sz.damaged_streams()["truncated_by_1"]
    assert shb.sz_decompress_range_host(cut, 100, 5000)[0] == 0 and shb.sz_decompress_range_host(cut, 29000, 1000)[0] != 0
    assert shb.sz_decompress_range_host(s, 0, 10, flags=2)[0] != 0
    assert shb.sz_decompress_range_host(b"", 0, 0)[0] != 0 and shb.sz_decompress_range_host(sz.IDENTIFIER, 0, 0)[:2] == (0, b"")


def test_gpu_sz_ranges_host_side_refusals_and_empty_calls(shb):
    import torch
    s = cases.streams()["mixed_20k"][0]
    n_chunks = len(cases.index_model(s)[1])
    ix = Index(shb, [s], n_chunks)
    L, vp = shb.lib(), lambda t: t.data_ptr()
    for seg in (64, 192, 255, 257, 1000):
        assert shb.sz_index_scratch_bytes(1, 100, seg, 100) == 0, seg
    assert shb.sz_index_scratch_bytes(4, 100, 0, 100) == shb.sz_index_scratch_bytes(4, 100, 1 << 20, 100) > \
        shb.sz_decompress_split_scratch_bytes(4, 100, 0, 100)
    need = shb.sz_index_scratch_bytes(1, n_chunks, 1024, 100)
    scratch = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    d_status = torch.full((2,), 0x55, dtype=torch.int32, device="cuda")
    d_result = torch.full((5,), 0x77, dtype=torch.int32, device="cuda")
    args = lambda **kw: [kw.get("items", vp(ix.d_items)), 1, n_chunks, kw.get("seg", 1024), 100, kw.get("chunks", vp(ix.d_chunks)),  # noqa: E731
                         kw.get("descs", vp(ix.d_descs)), kw.get("status", vp(d_status)), kw.get("result", vp(d_result)),
                         kw.get("scratch", vp(scratch)), kw.get("bytes", need), None]
    for bad in ({"items": None}, {"chunks": None}, {"descs": None}, {"status": None}, {"result": None}, {"scratch": None},
                {"scratch": vp(scratch) + 64}, {"bytes": need - 1}, {"seg": 1000}, {"seg": 128}):
        assert L.snappy_hip_sz_index_batch(*args(**bad)) == 2, bad                             # SNAPPY_HIP_ERR_ARG
    # the range call
    full = shb.sz_decompress_ranges_scratch_bytes(3)
    one = full - shb.sz_decompress_ranges_scratch_bytes(0) + 256 + 65536          # (an empty call's size: a 256-byte prefix and the slots)
    assert (shb.sz_decompress_ranges_scratch_bytes(0) - 256) % 65536 == 0
    rscratch = torch.empty(one + 256, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((64,), GUARD, dtype=torch.uint8, device="cuda")
    d_ranges = shb.make_ranges([(0, 0, 10, vp(d_dst)), (0, 5, 10, vp(d_dst) + 16), (0, 9, 10, vp(d_dst) + 32)])
    d_rstatus = torch.full((4,), 0x55, dtype=torch.int32, device="cuda")
    d_bad = torch.full((4,), 0x66, dtype=torch.int32, device="cuda")
    rargs = lambda **kw: [kw.get("descs", vp(ix.d_descs)), 1, kw.get("ranges", vp(d_ranges)), 3, kw.get("flags", 0), kw.get("status", vp(d_rstatus)),  # noqa: E731
                          kw.get("bad", vp(d_bad)), kw.get("scratch", vp(rscratch)), kw.get("bytes", one), None]
    for bad in ({"descs": None}, {"ranges": None}, {"status": None}, {"bad": None}, {"flags": 2}, {"scratch": None}, {"scratch": vp(rscratch) + 64},
                {"bytes": one - 1}):
        assert L.snappy_hip_sz_decompress_ranges(*rargs(**bad)) == 2, bad
    torch.cuda.synchronize()
    assert [int(x) for x in d_result.cpu().numpy()] == [0x77] * 5 and int(d_status.cpu()[0]) == 0x55       # nothing was enqueued
    assert [int(x) for x in d_rstatus.cpu().numpy()] == [0x55] * 4 and (d_dst.cpu().numpy() == GUARD).all()
    # exactly one slot is enough
    assert L.snappy_hip_sz_decompress_ranges(*rargs()) == 0
    torch.cuda.synchronize()
    plain = cases.streams()["mixed_20k"][1]
    assert [int(x) for x in d_rstatus.cpu().numpy()] == [0, 0, 0, 0x55]
    got = d_dst.cpu().numpy().tobytes()
    assert (got[:10], got[16:26], got[32:42]) == (plain[:10], plain[5:15], plain[9:19]) and got[10:16] == bytes([GUARD]) * 6
    # count == 0: OK, the four result words written; range_count == 0: OK, nothing written
    shb.sz_index_batch(ix.d_items, 0, 8, 0, 8, ix.d_chunks, ix.d_descs, d_status, d_result)
    torch.cuda.synchronize()
    assert [int(x) for x in d_result.cpu().numpy()] == [0, 0, 0, 0, 0x77]
    d_rstatus.fill_(0x55)
    shb.sz_decompress_ranges(ix.d_descs, 1, d_ranges, 0, d_rstatus, d_bad, d_scratch=rscratch)
    shb.sz_decompress_ranges(ix.d_descs, 0, d_ranges, 1, d_rstatus, d_bad, d_scratch=rscratch)            # no descs: every stream is out of bounds
    torch.cuda.synchronize()
    assert [int(x) for x in d_rstatus.cpu().numpy()] == [cases.OUT_OF_BOUNDS, 0x55, 0x55, 0x55]
