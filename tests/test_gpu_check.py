"""GPU tests (-m gpu) of the check through the C ABI (snappy_hip_check_blocks, snappy_hip_raw_check_batch, snappy_check_gpu,
snappy_check_raw_gpu, dpu_snappy -d -T).  The yardstick is the decoder on the same device: every per-block status is compared
with snappy_hip_decompress_blocks on the same stream and offsets, every raw verdict with snappy_hip_raw_decompress_batch, and
the four result words of a container with a plain fold over the decoder's statuses.  The check reads only: streams,
descriptors and items are byte-identical afterwards, and the words beside every array it writes keep their junk."""
import os

import numpy as np
import pytest

import datagen
import k2_window_cases as kc
import raw_cases as rc
from conftest import GOLDEN, GOLDEN_PAIRS, golden_bytes

pytestmark = pytest.mark.gpu

OK, INVALID, OUT_OF_BOUNDS, NONE = 0, 1, 2, 0xffffffff
JUNK = 0x5A5A5A5A            # what result words, status words and the words beside them hold before a call


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert binding.lib().snappy_hip_device_count() >= 1
    return binding


def fold(statuses):
    bad = [b for b, st in enumerate(statuses) if st != OK]
    return [INVALID if bad else OK, len(bad), bad[0] if bad else NONE, 0]


class Call:
    """One snappy_hip_check_blocks call over containers (stream, offsets, total_len, block_size): all streams in one device
    buffer, all offsets in another, every status array in one arena with a guard word in front of each and behind the last,
    the results between two guard words.  no_status: containers whose status pointer is null."""

    def __init__(self, shb, containers, no_status=()):
        import torch
        self.shb, self.containers = shb, containers
        n = len(containers)
        self.s_at, at = [], 0
        for s, _, _, _ in containers:
            self.s_at.append(at)
            at += (len(s) + 16 + 15) & ~15
        host = np.zeros(at + 16, dtype=np.uint8)
        for (s, _, _, _), o in zip(containers, self.s_at):
            host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.h_streams = host
        self.d_streams = torch.from_numpy(host).cuda()
        nbs = [len(c[1]) for c in containers]
        self.o_at = [int(x) for x in np.concatenate([[0], np.cumsum(nbs)])[:n]]
        self.d_offs = torch.from_numpy(np.array([o for c in containers for o in c[1]] + [0], dtype=np.int64)).cuda()
        self.st_at = [int(x) for x in (np.concatenate([[0], np.cumsum(np.array(nbs) + 1)])[:n] + 1)]
        self.st_words = sum(nbs) + n + 1
        self.d_status = torch.full((self.st_words,), JUNK, dtype=torch.int32, device="cuda")
        self.d_results = torch.full((4 * n + 2,), JUNK, dtype=torch.int32, device="cuda")
        self.d_index_result = torch.full((2 * n + 2,), JUNK, dtype=torch.int32, device="cuda")      # descriptors' `result`: not touched
        self.no_status = set(no_status)
        ptrs = [0 if i in self.no_status else self.d_status.data_ptr() + 4 * self.st_at[i] for i in range(n)]
        self.d_ptrs = torch.from_numpy(np.array(ptrs + [0], dtype=np.int64)).cuda()
        self.descs = shb.make_stream_descs(
            [dict(stream=self.d_streams[self.s_at[i]:], stream_len=len(c[0]), block_offsets=self.d_offs[self.o_at[i]:],
                  result=self.d_index_result[2 * i:], total_len=c[2], block_size=c[3], header_len=0, num_blocks=len(c[1]))
             for i, c in enumerate(containers)])
        self.h_descs = self.descs.cpu().numpy().copy()

    def run(self, with_status=True):
        import torch
        n = len(self.containers)
        self.shb.check_blocks(self.descs, n, self.d_results[1:], self.d_ptrs if with_status else None)
        torch.cuda.synchronize()
        res = self.d_results.cpu().numpy().view(np.uint32)
        assert res[0] == JUNK and res[-1] == JUNK, "a word beside the results was written"
        self.results = [[int(x) for x in res[1 + 4 * i:5 + 4 * i]] for i in range(n)]
        st = self.d_status.cpu().numpy().view(np.uint32)
        self.statuses = []
        for i, c in enumerate(self.containers):
            assert st[self.st_at[i] - 1] == JUNK, "the word in front of status array %d was written" % i
            self.statuses.append([int(x) for x in st[self.st_at[i]:self.st_at[i] + len(c[1])]])
        assert st[-1] == JUNK
        # read-only: streams, offsets' owner (the descriptors) and the index results as they were
        assert (self.d_streams.cpu().numpy() == self.h_streams).all()
        assert (self.descs.cpu().numpy() == self.h_descs).all()
        assert (self.d_index_result.cpu().numpy().view(np.uint32) == JUNK).all()
        return self

    def k2(self):
        """snappy_hip_decompress_blocks on every container, same stream, same offsets -> per-block statuses"""
        import torch
        d_out = torch.empty(max(c[2] for c in self.containers) + 64, dtype=torch.uint8, device="cuda")
        want = []
        for i, (s, offs, total, bs) in enumerate(self.containers):
            if not offs:
                want.append([])
                continue
            d_st = torch.full((len(offs),), 7, dtype=torch.int32, device="cuda")
            self.shb.decompress_blocks(self.d_streams[self.s_at[i]:], len(s), self.d_offs[self.o_at[i]:], total, bs, d_out, d_st)
            want.append([int(x) for x in d_st.cpu().numpy()])
        return want

    def compare(self, want):
        for i, w in enumerate(want):
            assert set(w) <= {OK, INVALID}, (i, w)
            if i in self.no_status:
                assert self.statuses[i] == [JUNK] * len(w), i
            else:
                assert self.statuses[i] == w, (i, self.statuses[i], w)
            assert self.results[i] == fold(w), (i, self.results[i], fold(w))


def damaged_streams(count=300):
    """The recipe of k2_window_cases.damaged_jobs: the damaged streams WHOLE, with the undamaged streams' offsets."""
    out = []
    r = np.random.default_rng(31337)
    for k in range(count):
        bs = int(r.choice([700, 4097, 32768]))
        stream, _ = datagen.element_stream(int(r.integers(2_000, 60_000)), bs, 40_000 + k, k % 4)
        total, _, offs = kc._offsets(stream)
        b = bytearray(stream)
        for _ in range(int(r.integers(1, 4))):
            at = int(r.integers(offs[0] + 4, len(b)))
            b[at] = int(r.integers(0, 256))
        out.append((bytes(b), offs, total, bs))
    return out


def test_block_statuses_and_results_against_k2_in_one_call(shb):
    """All intact containers, all 300 damaged streams and every hand-made block (a one-block container each) in ONE call of
    mixed block sizes, an empty container among them; every seventh container without a status array."""
    damaged = damaged_streams()
    jobs = {j[1] for j in kc.damaged_jobs(300)}
    assert jobs <= {d[0] for d in damaged} and len(jobs) >= 290                      # the same recipe: the same streams
    conts = []
    for _, s, _ in kc.intact_containers():
        total, bs, offs = kc._offsets(s)
        conts.append((s, offs, total, bs))
    conts += damaged
    conts += [(stream, [at], out_len, out_len) for _, stream, at, out_len in kc.hand_jobs()]
    empty = len(conts)
    conts.append((bytes.fromhex("00808002"), [], 0, 32768))
    call = Call(shb, conts, no_status=range(5, len(conts), 7))
    want = call.k2()
    call.run().compare(want)
    flat = [st for w in want for st in w]
    assert flat.count(OK) > 300 and flat.count(INVALID) > 300, (flat.count(OK), flat.count(INVALID))
    assert call.results[empty] == [OK, 0, NONE, 0]
    # the same call without any status array: the same results
    first = call.results
    call.run(with_status=False)
    assert call.results == first


def test_more_containers_than_one_trip_of_the_planner(shb):
    """1,031 containers (k2_window_cases.planner_trip_containers), the 1,025th with four blocks of which one is damaged:
    results and statuses against K2 per block."""
    conts = kc.planner_trip_containers()
    call = Call(shb, conts)
    want = call.k2()
    assert len(conts) > 1024 and want[1024] == [OK, OK, INVALID, OK] and sum(w == [INVALID] for w in want) > 90
    call.run().compare(want)


def test_malformed_descriptors_are_out_of_bounds_and_not_read(shb):
    import torch
    name, stream, _ = kc.intact_containers()[2]
    total, bs, offs = kc._offsets(stream)
    good = (stream, offs, total, bs)
    call = Call(shb, [good, good, good, good, good])
    d = call.descs.cpu().numpy().view(shb.STREAM_DESC_DTYPE).copy()
    d[1]["num_blocks"] += 1
    d[2]["block_size"] = 0
    d[3]["block_size"] = 65536
    d[4]["block_offsets"] = 0
    for k in (1, 2, 3, 4):                                    # nothing of them is read: their streams are claimed to be elsewhere
        d[k]["stream_len"] = 1 << 40
    call.descs = torch.from_numpy(d.view(np.uint8).copy()).cuda()
    call.h_descs = call.descs.cpu().numpy().copy()
    call.run()
    assert call.results[0] == [OK, 0, NONE, 0] and call.statuses[0] == [OK] * len(offs)
    for k in (1, 2, 3, 4):
        assert call.results[k] == [OUT_OF_BOUNDS, 0, NONE, 0], k
        assert call.statuses[k] == [JUNK] * len(offs), k


def test_arguments(shb):
    import torch
    name, stream, _ = kc.intact_containers()[0]
    total, bs, offs = kc._offsets(stream)
    call = Call(shb, [(stream, offs, total, bs)])
    lib = shb.lib()
    assert lib.snappy_hip_check_blocks(None, 0, None, None, None, 0, None) == 0              # count == 0: OK, nothing launched
    assert lib.snappy_hip_raw_check_batch(None, 0, None, None, None) == 0
    scratch = torch.empty(1024, dtype=torch.uint8, device="cuda")
    assert shb.check_scratch_bytes(1) == 256 and shb.check_scratch_bytes(31) == 512
    args = (call.descs.data_ptr(), 1, None, call.d_results.data_ptr(), scratch.data_ptr(), 512, None)
    for k, v in ((0, None), (3, None), (4, None), (4, scratch.data_ptr() + 64), (5, 255)):
        bad = list(args)
        bad[k] = v
        assert lib.snappy_hip_check_blocks(*bad) == 2, k                                        # SNAPPY_HIP_ERR_ARG
    assert lib.snappy_hip_raw_check_batch(None, 1, None, None, None) == 2
    torch.cuda.synchronize()
    assert (call.d_results.cpu().numpy().view(np.uint32) == JUNK).all()
    assert lib.snappy_hip_check_blocks(*args) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in call.d_results.cpu().numpy().view(np.uint32)[:4]] == [OK, 0, NONE, 0]


@pytest.fixture(scope="module")
def megabyte_of_small_blocks(shb):
    """1 MiB at 64-byte blocks: 16,384 blocks, more than the wavefronts resident on the device, so wavefronts draw repeatedly"""
    import torch
    plain = datagen.lz_structured(1 << 20, 77)
    d_in = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
    stream = bytes(shb.compress_resident(d_in, 64).cpu().numpy())
    total, bs, offs = kc._offsets(stream)
    assert (total, bs, len(offs)) == (1 << 20, 64, 16384)
    return stream, offs, total, bs


def test_more_blocks_than_wavefronts_intact(shb, megabyte_of_small_blocks):
    call = Call(shb, [megabyte_of_small_blocks])
    want = call.k2()
    assert want[0] == [OK] * 16384
    call.run().compare(want)


def test_more_blocks_than_wavefronts_with_100_damaged_bytes(shb, megabyte_of_small_blocks):
    stream, offs, total, bs = megabyte_of_small_blocks
    b = bytearray(stream)
    r = np.random.default_rng(2718)
    for _ in range(100):
        b[int(r.integers(offs[0], len(b)))] ^= int(r.integers(1, 256))
    call = Call(shb, [(bytes(b), offs, total, bs)])
    want = call.k2()
    assert 1 <= want[0].count(INVALID) <= 100             # (a changed byte damages at most its own block; a changed size word or tag, some)
    call.run().compare(want)


def test_goldens_are_ok_resident_and_through_the_drop_in_call(shb):
    import torch
    for name in GOLDEN_PAIRS:
        s = golden_bytes(name + ".snappy")
        d = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).cuda()
        assert shb.check_resident(d) == (True, 0, None), name
        st, rep, rt = shb.check_host(s)
        nb = len(kc._offsets(s)[2])
        assert st == 0 and rep == dict(blocks=nb, bad_blocks=0, first_bad_block=(1 << 64) - 1, first_bad_offset=(1 << 64) - 1), (name, rep)
        assert rt["run"] > 0 and rt["copy_in"] > 0 and rt["copy_out"] > 0 and rt["d_alloc"] > 0
    # a damaged golden: blocks 1 and 3 of terror2 start with a copy
    s = golden_bytes("terror2.snappy")
    _, _, offs = kc._offsets(s)
    b = bytearray(s)
    b[offs[1] + 4] = b[offs[3] + 4] = 0xFF
    d = torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()
    assert shb.check_resident(d) == (False, 2, 1)
    st, rep, _ = shb.check_host(bytes(b))
    assert st == 1 and rep == dict(blocks=4, bad_blocks=2, first_bad_block=1, first_bad_offset=offs[1])
    # a broken chain is decided on the host
    st, rep, rt = shb.check_host(s[:offs[2] + 9])
    assert st == 1 and rep == dict(blocks=4, bad_blocks=1, first_bad_block=2, first_bad_offset=offs[2]) and rt["run"] == 0
    assert shb.check_resident(d[:offs[2] + 9])[0] is False
    st, rep, _ = shb.check_host(bytes.fromhex("00808002"))
    assert st == 0 and rep["blocks"] == 0


def test_raw_vectors_and_fixtures_against_the_decoder(shb):
    import torch
    from test_gpu_raw import Batch
    streams = list(rc.intact_vectors().values()) + list(rc.damaged_vectors().values()) + [rc.fixture_stream(n) for n in rc.FIXTURES]
    big = rc.varint(rc.RAW_MAX_LEN + 1) + rc.literal(b"x")
    items = []
    for s in streams + [big]:
        h = rc.header_parses(s)
        n = h[0] if h and h[0] <= (1 << 22) else 0
        items.append((s, n))
    some = rc.intact_vectors()["all_types"]
    items.append((some, 3000, 1))                              # a null src
    items.append((some, 3400, 0, rc.RAW_MAX_LEN + 1))          # a claimed src_len above the maximum (never read that far)
    dec = Batch(items)
    shb.raw_decompress_batch(shb.make_raw_items(dec.entries), dec.n, dec.d_out_len, dec.d_status)
    dec.fetch()
    chk = Batch(items)
    # dst and dst_capacity are ignored: give the check none
    entries = [(e[0], e[1], 0, 0) for e in chk.entries]
    d_items = shb.make_raw_items(entries)
    h_items = d_items.cpu().numpy().copy()
    h_src = chk.d_src.cpu().numpy().copy()
    shb.raw_check_batch(d_items, chk.n, chk.d_out_len, chk.d_status)
    chk.fetch()                                                # (asserts the words behind both arrays and every guard byte)
    assert (d_items.cpu().numpy() == h_items).all() and (chk.d_src.cpu().numpy() == h_src).all()
    assert (chk.buf == rc.GUARD).all()                         # not one byte of any dst
    for i, it in enumerate(items):
        assert (chk.status[i], chk.out_len[i]) == (dec.status[i], dec.out_len[i]), (i, chk.status[i], chk.out_len[i], dec.status[i], dec.out_len[i])
        assert chk.status[i] != rc.DST_TOO_SMALL
    for i, s in enumerate(streams):
        assert (chk.status[i], chk.out_len[i]) == rc.expect(s)[:2], i
    assert sorted(set(chk.status[:chk.n])) == [rc.OK, rc.INVALID, rc.TOO_LARGE]
    # the drop-in call
    for name in rc.FIXTURES:
        st, n, rt = shb.check_raw_host(rc.fixture_stream(name))
        assert (st, n) == (0, len(rc.fixture_plain(name))) and rt["run"] > 0, name
    s = rc.fixture_stream("terror2")
    assert shb.check_raw_host(s[:len(s) // 2])[0] == 1 and shb.check_raw_host(b"")[:2] == (1, 0)


def test_raw_check_of_damaged_rich_streams_against_the_independent_decoder(shb):
    """600 seeded mutations of streams no greedy compressor writes (tests/raw_split_cases.damaged_rich_streams): the check's
    (status, out_len) equals raw_cases.expect, the format's CPU statement, on every one."""
    import raw_split_cases as sc
    from test_gpu_raw import Batch
    items = sc.damaged_rich_streams()
    want = [rc.expect(s, n)[:2] for s, n in items]
    assert len(items) == 600 and [w[0] for w in want].count(rc.OK) >= 100 and [w[0] for w in want].count(rc.INVALID) >= 100
    chk = Batch([(s, 0) for s, _ in items])
    shb.raw_check_batch(shb.make_raw_items([(e[0], e[1], 0, 0) for e in chk.entries]), chk.n, chk.d_out_len, chk.d_status)
    chk.fetch()
    assert list(zip(chk.status, chk.out_len))[:chk.n] == want, [(i, chk.status[i], chk.out_len[i], w) for i, w in enumerate(want)
                                                                  if (chk.status[i], chk.out_len[i]) != w][:5]


def test_cli_check_on_the_device(shb, tmp_path):
    from test_cli import run
    import subprocess
    from test_cli import CLI, HOST_DIR
    subprocess.check_call(["make", "-s", "-C", HOST_DIR])
    s = golden_bytes("terror2.snappy")
    _, _, offs = kc._offsets(s)
    r = run(CLI, "-d", "-T", "-i", os.path.join(GOLDEN, "terror2.snappy"))
    assert r.returncode == 0 and "Check: OK, 4 blocks\n" in r.stdout, (r.stdout, r.stderr)
    b = bytearray(s)
    b[offs[1] + 4] = b[offs[3] + 4] = 0xFF
    bad = tmp_path / "bad.snappy"
    bad.write_bytes(bytes(b))
    r = run(CLI, "-d", "-T", "-i", str(bad))
    assert r.returncode == 1 and "Check: INVALID, 2 of 4 blocks, first bad block 1 at offset %d\n" % offs[1] in r.stdout, (r.stdout, r.stderr)
    raw = os.path.join(GOLDEN, "raw", "terror2.raw_snappy")
    r = run(CLI, "-d", "-T", "-R", "-i", raw)
    assert r.returncode == 0 and "Check: OK, 105438 bytes\n" in r.stdout, (r.stdout, r.stderr)
    cut = tmp_path / "cut.raw_snappy"
    cut.write_bytes(rc.fixture_stream("terror2")[:40000])
    r = run(CLI, "-d", "-T", "-R", "-i", str(cut))
    assert r.returncode == 1 and "Check: INVALID\n" in r.stdout, (r.stdout, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["bad.snappy", "cut.raw_snappy"]
