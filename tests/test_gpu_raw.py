"""GPU tests (-m gpu) of the raw Snappy batch interface through the C ABI (snappy_hip_raw_decompress_batch /
snappy_hip_raw_compress_batch): the vectors and third-party fixtures of tests/test_raw_emulated.py on the device with guard
bytes around every dst, a batch of 16,384 items carved from a 1 GiB Silesia-mix, and the generated code.  All comparisons
are exact."""
import os
import re
import subprocess

import numpy as np
import pytest

import datagen
import oracle_lib as oracle
import raw_cases as rc
from conftest import golden_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 37                       # guard bytes in front of every dst (odd: destinations and sources land on every alignment)


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert binding.lib().snappy_hip_device_count() >= 1
    return binding


class Batch:
    """items: list of (src bytes, capacity) or (src bytes, capacity, flags, src_len) as tests/emu_raw_lib.Batch takes them.
    All sources in one device buffer (GAP bytes apart), all destinations in another, filled with rc.GUARD."""

    def __init__(self, items):
        import torch
        self.items = items
        srcs = [it[0] for it in items]
        self.src_at = np.cumsum([GAP + len(s) for s in srcs]) - np.array([len(s) for s in srcs], dtype=np.int64) if items else np.zeros(0, np.int64)
        blob = bytearray()
        for s in srcs:
            blob += bytes(GAP) + s
        self.d_src = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(GAP), dtype=np.uint8).copy()).cuda()
        caps = np.array([int(it[1]) for it in items], dtype=np.int64)
        self.caps = caps
        self.dst_at = np.cumsum(caps + GAP) - caps if items else np.zeros(0, np.int64)
        self.buf_len = int(self.dst_at[-1] + caps[-1] + GAP) if items else GAP
        self.d_dst = torch.full((self.buf_len,), rc.GUARD, dtype=torch.uint8, device="cuda")
        entries = []
        for i, it in enumerate(items):
            flags = it[2] if len(it) > 2 else 0
            entries.append((0 if flags & 1 else self.d_src.data_ptr() + int(self.src_at[i]), it[3] if len(it) > 3 else len(it[0]),
                            0 if flags & 2 else self.d_dst.data_ptr() + int(self.dst_at[i]), int(it[1])))
        self.entries = entries
        self.n = len(items)
        self.d_out_len = torch.full((self.n + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        self.d_status = torch.full((self.n + 1,), 0x55, dtype=torch.int32, device="cuda")
        self.d_result = torch.full((2,), 0x77, dtype=torch.int32, device="cuda")

    def fetch(self):
        import torch
        torch.cuda.synchronize()
        self.status = [int(x) for x in self.d_status.cpu().numpy()]
        self.out_len = [int(x) for x in self.d_out_len.cpu().numpy()]
        self.result = [int(x) for x in self.d_result.cpu().numpy()]
        self.buf = self.d_dst.cpu().numpy()
        assert self.status[self.n] == 0x55 and self.out_len[self.n] == 0x5A5A5A5A5A5A5A5A
        # the guard bytes between, in front of and behind the windows
        for i in range(self.n):
            assert (self.buf[int(self.dst_at[i]) - GAP:int(self.dst_at[i])] == rc.GUARD).all(), i
        assert (self.buf[self.buf_len - GAP:] == rc.GUARD).all()

    def window(self, i):
        return self.buf[int(self.dst_at[i]):int(self.dst_at[i] + self.caps[i])].tobytes()


def gpu_decompress(shb, items):
    b = Batch(items)
    shb.raw_decompress_batch(shb.make_raw_items(b.entries), b.n, b.d_out_len, b.d_status)
    b.fetch()
    return b


def gpu_compress(shb, items, block_size, max_fragments):
    b = Batch(items)
    shb.raw_compress_batch(shb.make_raw_items(b.entries), b.n, block_size, max_fragments, b.d_out_len, b.d_status, b.d_result)
    b.fetch()
    return b


FILL = bytes([rc.GUARD])


def check_decoded(b, i, s, capacity):
    st, n, plain = rc.expect(s, capacity)
    assert (b.status[i], b.out_len[i]) == (st, n), (i, b.status[i], b.out_len[i], st, n)
    w = b.window(i)
    if st == rc.OK:
        assert w[:n] == plain and w[n:] == FILL * (capacity - n), i
    elif st != rc.INVALID or n == 0:
        assert w == FILL * capacity, i
    else:
        assert w[n:] == FILL * (capacity - n), i          # INVALID: only dst[0, length) is unspecified


def test_gpu_raw_decode_fixtures_and_vectors_in_one_batch(shb):
    """Every third-party fixture, every intact and every damaged vector, each at capacities exact, generous and one short, in
    one launch."""
    streams = [rc.fixture_stream(n) for n in rc.FIXTURES] + list(rc.intact_vectors().values()) + list(rc.damaged_vectors().values())
    items = []
    for s in streams:
        h = rc.header_parses(s)
        n = h[0] if h else 0
        for cap in (n, n + 5) + ((n - 1,) if n else ()):
            items.append((s, cap))
    b = gpu_decompress(shb, items)
    for i, (s, cap) in enumerate(items):
        check_decoded(b, i, s, cap)
    for k, name in enumerate(rc.FIXTURES):
        assert b.status[3 * k] == rc.OK and b.window(3 * k) == rc.fixture_plain(name), name
    assert sorted(set(b.status[:b.n])) == [rc.OK, rc.INVALID, rc.DST_TOO_SMALL]


def test_gpu_raw_decode_damaged_rich_streams_against_the_independent_decoder(shb):
    """600 seeded mutations of streams no greedy compressor writes (tests/raw_split_cases.damaged_rich_streams) in one launch:
    (status, out_len) equals raw_cases.expect, accepted bytes are decode_raw's, nothing behind dst[length)."""
    import raw_split_cases as sc
    items = sc.damaged_rich_streams()
    verdicts = [rc.expect(s, n)[0] for s, n in items]
    assert len(items) == 600 and verdicts.count(rc.OK) >= 100 and verdicts.count(rc.INVALID) >= 100
    b = gpu_decompress(shb, items)
    for i, (s, n) in enumerate(items):
        check_decoded(b, i, s, n)


def test_gpu_raw_decode_alone_and_limits(shb):
    import torch
    lit = rc.intact_vectors()["literal_65537"]
    b = gpu_decompress(shb, [(lit, 65537)])
    assert b.status[0] == rc.OK and b.window(0) == rc.trs.decode_raw(lit)       # (a block decoder's 64 KiB literal bound refuses it)
    s = rc.intact_vectors()["all_types"]
    n = rc.header_parses(s)[0]
    b = gpu_decompress(shb, [(s, 0, 2), (s, n, 2), (s, n, 1), (s, n, 0, rc.RAW_MAX_LEN + 1), (rc.varint(rc.RAW_MAX_LEN + 1) + b"\x00x", 16),
                             (rc.varint(rc.RAW_MAX_LEN) + b"\x00x", 16), (b"\x00", 0, 2), (b"\x00", 0)])
    assert list(zip(b.status, b.out_len))[:8] == [(rc.DST_TOO_SMALL, n), (rc.DST_TOO_SMALL, n), (rc.INVALID, 0), (rc.TOO_LARGE, n),
                                                  (rc.TOO_LARGE, rc.RAW_MAX_LEN + 1), (rc.DST_TOO_SMALL, rc.RAW_MAX_LEN), (rc.OK, 0), (rc.OK, 0)]
    assert (b.buf == rc.GUARD).all()
    assert shb.RAW_MAX_LEN == rc.RAW_MAX_LEN >= 1 << 30
    # count == 0 launches nothing; null arrays with items are refused on the host
    shb.raw_decompress_batch(torch.zeros(32, dtype=torch.uint8, device="cuda"), 0, torch.zeros(1, dtype=torch.int64, device="cuda"),
                             torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert shb.lib().snappy_hip_raw_decompress_batch(None, 1, None, None, None) == 2
    assert shb.lib().snappy_hip_raw_decompress_batch(None, 0, None, None, None) == 0


def want_raw(plain, bs):
    return rc.trs.convert(oracle.compress(plain, bs))


def check_compressed(b, i, want, capacity):
    w = b.window(i)
    if len(want) <= capacity:
        assert (b.status[i], b.out_len[i]) == (rc.OK, len(want)), (i, b.status[i], b.out_len[i], len(want))
        assert w[:len(want)] == want and w[len(want):] == FILL * (capacity - len(want)), i
    else:
        assert (b.status[i], b.out_len[i]) == (rc.DST_TOO_SMALL, len(want)) and w == FILL * capacity, i
    return len(want) <= capacity


@pytest.mark.parametrize("bs", [64, 1000, 32768, 65535])
def test_gpu_raw_compress_items_around_a_fragment(shb, bs, monkeypatch):
    text = golden_bytes("plrabn12.txt")
    lengths = rc.compress_lengths(bs) + [7 * bs + 5, 300000]
    plains = [b"" if not n else datagen.text_random_interleave(text, n, seed=bs + k) if k % 3 else datagen.lz_structured(n, bs + k)
              for k, n in enumerate(lengths)]
    wants = [want_raw(p, bs) for p in plains]
    frags = sum((len(p) + bs - 1) // bs for p in plains)
    caps = [len(w) - 1 if i in (2, 5) else (len(w) if i % 2 else shb.raw_compress_bound(len(plains[i]), bs)) for i, w in enumerate(wants)]
    assert all(shb.raw_compress_bound(len(p), bs) >= len(w) for p, w in zip(plains, wants))
    for form in ("1", "0"):                              # both forms of K1's parse (bit 0: the stream form of the LDS-table kernel)
        monkeypatch.setenv("SNAPPY_HIP_K1_STREAM", form)
        b = gpu_compress(shb, list(zip(plains, caps)), bs, frags)
        ok = sum(check_compressed(b, i, w, caps[i]) for i, w in enumerate(wants))
        assert b.result == [frags, ok] and ok == len(plains) - 2
    monkeypatch.delenv("SNAPPY_HIP_K1_STREAM")
    # one slot short: the last item with fragments is TOO_LARGE, the others complete, d_result[0] = the need
    b = gpu_compress(shb, list(zip(plains, caps)), bs, frags - 1)
    last = max(i for i, p in enumerate(plains) if p)
    for i, w in enumerate(wants):
        if i == last:
            assert (b.status[i], b.out_len[i]) == (rc.TOO_LARGE, 0) and b.window(i) == FILL * caps[i]
        else:
            check_compressed(b, i, w, caps[i])
    assert b.result[0] == frags
    # the new decoder reads what the compressor wrote
    d = gpu_decompress(shb, [(w, len(p)) for w, p in zip(wants, plains)])
    for i, p in enumerate(plains):
        assert d.status[i] == rc.OK and d.window(i) == p, i


def test_gpu_raw_compress_one_item_more_than_a_planner_trip(shb):
    """raw_plan_kernel takes 1024 items per trip of its loop: 1025 items of one fragment each, so the last item's fragment is
    numbered from the carry of the first trip."""
    bs = 1000
    text = golden_bytes("plrabn12.txt")
    plains = [text[37 * k:37 * k + 1 + (k * 7919) % bs] for k in range(1025)]
    assert all(0 < len(p) <= bs for p in plains) and len(plains[1024]) > 1
    wants = [want_raw(p, bs) for p in plains]
    caps = [len(w) + k % 3 for k, w in enumerate(wants)]
    b = gpu_compress(shb, list(zip(plains, caps)), bs, 1025)
    for i, w in enumerate(wants):
        assert check_compressed(b, i, w, caps[i]), i
    assert b.result == [1025, 1025]


def test_gpu_raw_compress_goldens_bad_items_and_arguments(shb):
    import torch
    names = ["alice", "coding", "terror2", "plrabn12", "world192"]
    plains = [golden_bytes(n + ".txt") for n in names]
    wants = [rc.trs.convert(golden_bytes(n + ".snappy")) for n in names]
    b = gpu_compress(shb, [(p, len(w)) for p, w in zip(plains, wants)], 32768, 64)
    for i, w in enumerate(wants):
        assert b.status[i] == rc.OK and b.window(i) == w, names[i]
    b = gpu_compress(shb, [(b"abc", 16, 1), (b"", 1, 1, 0), (b"abc", 16, 0, 1 << 32), (b"abcd" * 10, 0, 2), (b"", 0)], 1000, 8)
    assert b.status[:5] == [rc.INVALID, rc.OK, rc.TOO_LARGE, rc.DST_TOO_SMALL, rc.DST_TOO_SMALL]
    assert b.window(1) == b"\x00" and b.out_len[:5] == [0, 1, 0, len(want_raw(b"abcd" * 10, 1000)), 1] and b.result == [1, 1]
    L = shb.lib()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    need = shb.raw_compress_scratch_bytes(1000, 1, 4)
    assert need > 0 and shb.raw_compress_scratch_bytes(0, 1, 4) == 0 and shb.raw_compress_bound(10, 65536) == 0
    big = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    sp = (big.data_ptr() + 255) & ~255
    for args in ((None, 1, 1000, 4, p, p, p, sp, need, None), (p, 1, 0, 4, p, p, p, sp, need, None), (p, 1, 65536, 4, p, p, p, sp, need, None),
                 (p, 1, 1000, 4, p, p, p, sp + 16, need, None), (p, 1, 1000, 4, p, p, p, sp, need - 1, None), (p, 1, 1000, 4, p, p, None, sp, need, None)):
        assert L.snappy_hip_raw_compress_batch(*args) == 2, args


def test_gpu_raw_silesia_mix_16384_items(shb):
    """16,384 items carved from a resident 1 GiB Silesia-mix at seeded lengths of 1 B .. 1 MiB (log-uniform), compressed at
    32 KiB fragments: every item's stream against the oracle-derived bytes, then decoded again against the plaintext."""
    import torch
    import silesia_mix
    bs = 32768
    st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(golden_bytes("xml.snappy"), dtype=np.uint8).copy()).cuda())
    assert st == 0
    unit = silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0)
    n = 1 << 30
    d_in = silesia_mix.container_from_unit(torch.from_numpy(unit.copy()).cuda(), n)
    host = d_in[:n].cpu().numpy()
    rng = np.random.default_rng(2025)
    count = 16384
    lengths = np.clip(np.exp(rng.uniform(0.0, np.log(float(1 << 20)), count)).astype(np.int64), 1, 1 << 20)
    offsets = (rng.random(count) * (n - lengths + 1)).astype(np.int64)
    caps = np.array([shb.raw_compress_bound(int(k), bs) for k in lengths], dtype=np.int64)
    dst = np.cumsum(caps + GAP) - caps
    buf_len = int(dst[-1] + caps[-1] + GAP)
    buf = torch.full((buf_len,), rc.GUARD, dtype=torch.uint8, device="cuda")
    frags = int(((lengths + bs - 1) // bs).sum())
    d_items = shb.make_raw_items([(d_in.data_ptr() + int(o), int(k), buf.data_ptr() + int(d), int(c)) for o, k, d, c in zip(offsets, lengths, dst, caps)])
    d_len = torch.zeros(count, dtype=torch.int64, device="cuda")
    d_status = torch.full((count,), 0x55, dtype=torch.int32, device="cuda")
    d_result = torch.zeros(2, dtype=torch.int32, device="cuda")
    shb.raw_compress_batch(d_items, count, bs, frags, d_len, d_status, d_result)
    torch.cuda.synchronize()
    assert [int(x) for x in d_result.cpu().numpy()] == [frags, count]
    assert int((d_status != 0).sum().item()) == 0
    out_len = d_len.cpu().numpy()
    got = buf.cpu().numpy()
    for i in range(count):
        want = want_raw(host[int(offsets[i]):int(offsets[i] + lengths[i])].tobytes(), bs)
        at = int(dst[i])
        assert int(out_len[i]) == len(want) and got[at:at + len(want)].tobytes() == want, i
        assert (got[at - GAP:at] == rc.GUARD).all() and (got[at + len(want):at + int(caps[i])] == rc.GUARD).all(), i
    assert (got[buf_len - GAP:] == rc.GUARD).all()
    # decode the streams where they lie, into a second buffer of exactly the plaintext lengths behind guard gaps
    pdst = np.cumsum(lengths + GAP) - lengths
    plain_len = int(pdst[-1] + lengths[-1] + GAP)
    pbuf = torch.full((plain_len,), rc.GUARD, dtype=torch.uint8, device="cuda")
    d_items2 = shb.make_raw_items([(buf.data_ptr() + int(d), int(k), pbuf.data_ptr() + int(p), int(m)) for d, k, p, m in zip(dst, out_len, pdst, lengths)])
    d_len2 = torch.zeros(count, dtype=torch.int64, device="cuda")
    d_status2 = torch.full((count,), 0x55, dtype=torch.int32, device="cuda")
    shb.raw_decompress_batch(d_items2, count, d_len2, d_status2)
    torch.cuda.synchronize()
    assert int((d_status2 != 0).sum().item()) == 0 and bool((d_len2.cpu() == torch.from_numpy(lengths)).all().item())
    bad = [i for i in range(count) if not torch.equal(pbuf[int(pdst[i]):int(pdst[i] + lengths[i])], d_in[int(offsets[i]):int(offsets[i] + lengths[i])])]
    assert bad == [], bad[:10]
    gaps = torch.from_numpy((pdst[:, None] - GAP + np.arange(GAP)[None, :]).reshape(-1)).cuda()
    assert bool((pbuf[gaps] == rc.GUARD).all().item()) and bool((pbuf[plain_len - GAP:] == rc.GUARD).all().item())


def test_raw_kernels_use_global_not_flat_instructions(tmp_path):
    """raw_decompress_kernel runs K2's decoder, which relies on global_* operations of one wavefront completing in issue order
    (tests/test_abi_symbols.py); its pointers come from items in memory, so the check is repeated on its code -- and on the
    compress kernels, whose K1 parse relies on the same guarantee."""
    import __graft_entry__ as entry
    src = os.path.join(ROOT, "pim-compression_amd", "csrc", "snappy_hip.hip")
    asm = tmp_path / "device.s"
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(asm)])
    text = asm.read_text()
    for name, least in (("raw_decompress_kernel", 20), ("raw_compress_fragments_kernel", 10), ("raw_sizes_kernel", 5), ("raw_gather_kernel", 5)):
        found = re.findall(r"^(_ZN10snappy_hip\d+" + name + r"\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
        assert found, name
        for _, body in found:
            assert re.findall(r"^\s*flat_\w+", body, re.M) == [], name
            assert len(re.findall(r"^\s*global_(?:load|store|atomic)", body, re.M)) >= least, name


# ---- drop-in level and CLI: snappy_compress_raw_gpu / snappy_decompress_raw_gpu and dpu_snappy -d -R against host mode ----

def _cli(args, tmp_path, tag):
    from test_cli import CLI, HOST_DIR
    subprocess.check_call(["make", "-s", "-C", HOST_DIR])
    out = tmp_path / tag
    r = subprocess.run([CLI, *args, "-o", str(out)], capture_output=True, text=True)
    return r, (out.read_bytes() if out.exists() else None)


def test_gpu_raw_dropin_and_cli_match_host_mode(shb, tmp_path):
    from test_cli import check_stdout_contract
    for name in ("alice", "terror2", "world192"):
        plain = golden_bytes(name + ".txt")
        src = os.path.join(ROOT, "tests", "golden", name + ".txt")
        for bs in (1000, 32768):
            want = want_raw(plain, bs)
            st, got, rt = shb.raw_compress_host(plain, bs)
            assert st == 0 and got == want, (name, bs)
            assert set(rt) >= {"pre", "d_alloc", "load", "copy_in", "run", "copy_out", "d_free"}
            r_h, host = _cli(["-c", "-R", "-b", str(bs), "-i", src], tmp_path, "h")
            r_d, dev = _cli(["-d", "-c", "-R", "-b", str(bs), "-i", src], tmp_path, "d")
            assert r_h.returncode == 0 and r_d.returncode == 0, (r_h.stderr, r_d.stderr)
            check_stdout_contract(r_d.stdout)
            assert host == dev == want, (name, bs)
    streams = {n: rc.fixture_stream(n) for n in rc.FIXTURES}
    streams.update(rc.intact_vectors())
    for name, s in streams.items():
        plain = rc.trs.decode_raw(s)
        st, got, rt = shb.raw_decompress_host(s)
        assert st == 0 and got == plain, name
        assert set(rt) >= {"pre", "d_alloc", "load", "copy_in", "run", "copy_out", "d_free"}
        path = tmp_path / (name + ".raw_snappy")
        path.write_bytes(s)
        r_h, host = _cli(["-R", "-i", str(path)], tmp_path, "h_" + name)
        r_d, dev = _cli(["-d", "-R", "-i", str(path)], tmp_path, "d_" + name)
        assert r_h.returncode == 0 and r_d.returncode == 0, (name, r_h.stderr, r_d.stderr)
        assert host == dev == plain, name
    for name, s in rc.damaged_vectors().items():
        st, got, _ = shb.raw_decompress_host(s)
        assert st == shb.SNAPPY_INVALID_INPUT and got == b"", name
    path = tmp_path / "damaged.raw_snappy"
    path.write_bytes(rc.damaged_vectors()["offset_0"])
    r_d, dev = _cli(["-d", "-R", "-i", str(path)], tmp_path, "damaged.out")
    assert r_d.returncode != 0 and r_d.stderr.strip() and dev is None
    # caller-owned output buffers: exact, one short
    s = rc.fixture_stream("coding")
    plain = rc.fixture_plain("coding")
    assert shb.raw_decompress_host(s, out_capacity=len(plain))[:2] == (0, plain)
    assert shb.raw_decompress_host(s, out_capacity=len(plain) - 1)[0] == shb.SNAPPY_BUFFER_TOO_SMALL
    want = want_raw(plain, 32768)
    assert shb.raw_compress_host(plain, 32768, out_capacity=len(want))[:2] == (0, want)
    assert shb.raw_compress_host(plain, 32768, out_capacity=len(want) - 1)[0] == shb.SNAPPY_BUFFER_TOO_SMALL
    assert shb.raw_compress_host(b"", 32768)[:2] == (0, b"\x00")
    assert shb.raw_decompress_host(b"\x00")[:2] == (0, b"")
