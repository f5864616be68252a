"""GPU tests (-m gpu) of the container resize through the C ABI (snappy_hip_resize) and the binding: the matrix of
tests/test_resize_emulated.py on the device, the reference's goldens, an append of many more blocks than the recompress kernel
has wavefronts, a chain of resizes and an update without host synchronisation, the drop-in call and the CLI.  The check is an
identity with no tolerance: the new stream == oracle.compress(plaintext[:keep_len] + the segments' bytes)."""
import os
import subprocess

import numpy as np
import pytest

import datagen
import oracle_lib as oracle
import ranges_cases as rc
import resize_cases as rz
import update_cases as uc
from conftest import golden_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
GUARD64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert binding.lib().snappy_hip_device_count() >= 1
    return binding


def _dev_bytes(data):
    import torch
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if len(data) else torch.zeros(1, dtype=torch.uint8, device="cuda")


class Result:
    pass


def gpu_resize(shb, c, keep_len, segments, new_total=None, capacity=None, stream=None, desc_shape=None):
    """As test_resize_emulated.run, on the device.  segments: list of bytes or (data, length, null src)."""
    import torch
    nb, bs = c.num_blocks, c.block_size
    old = c.stream if stream is None else stream
    d_stream = _dev_bytes(old)
    d_off = torch.from_numpy(np.ascontiguousarray(c.offsets if nb else np.zeros(1), dtype=np.uint64).view(np.int64)).cuda()
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    dt, dbs, dnb = desc_shape or (c.total, bs, nb)
    d_desc = shb.make_stream_descs([dict(stream=d_stream, stream_len=len(old), block_offsets=d_off, result=d_res, total_len=dt,
                                         block_size=dbs, header_len=c.header_len, num_blocks=dnb)])
    # the sources packed into one buffer, every one behind i % 16 + 1 spare bytes (all alignments)
    packed, entries, total = bytearray(), [], keep_len
    for i, s in enumerate(segments):
        data, length, null = (s, len(s), False) if isinstance(s, bytes) else s
        packed += bytes(i % 16 + 1)
        entries.append((None if null else len(packed), length))
        packed += data
        total += length
    d_src = _dev_bytes(bytes(packed) + b"\0")
    d_segments = shb.make_segments([(0 if at is None else d_src.data_ptr() + at, n) for at, n in entries])
    if new_total is None:
        new_total = total
    new_nb = shb.num_blocks(new_total, bs)
    if capacity is None:
        capacity = 10 + new_nb * shb.slot_stride(bs)
    out = torch.full((capacity + 2 * PAD,), rz.GUARD, dtype=torch.uint8, device="cuda")
    new_offs = torch.from_numpy(np.full(new_nb + 3, GUARD64, dtype=np.uint64).view(np.int64)).cuda()
    new_len = torch.from_numpy(np.full(1, GUARD64, dtype=np.uint64).view(np.int64)).cuda()
    result = torch.full((2,), 0x77, dtype=torch.int32, device="cuda")
    status = torch.full((max(len(segments), 1),), 0x55, dtype=torch.int32, device="cuda")
    shb.resize(d_desc, c.total, bs, keep_len, new_total, d_segments, len(segments), status, out[PAD:], new_offs[1:], new_len, result,
               capacity=capacity)
    torch.cuda.synchronize()
    r = Result()
    r.old_unchanged = bytes(d_stream.cpu().numpy()[:len(old)]) == old
    r.status = [int(x) for x in status.cpu().numpy()[:len(segments)]]
    r.result = [int(x) for x in result.cpu().numpy()]
    r.new_len = int(new_len.cpu().numpy().view(np.uint64)[0])
    r.out = out.cpu().numpy()
    r.new_offs, r.new_nb = new_offs.cpu().numpy().view(np.uint64), new_nb
    r.stream = r.out[PAD:PAD + r.new_len].tobytes() if r.new_len <= capacity else None
    return r


def assert_untouched(r):
    assert r.old_unchanged
    assert r.result[0] == rz.REJECTED, r.result
    assert r.new_len == 0
    assert (r.out == rz.GUARD).all()
    assert (r.new_offs == GUARD64).all()


def check_ok(shb, c, keep_len, segments, want=None, **kw):
    r = gpu_resize(shb, c, keep_len, segments, **kw)
    stream, want_offs, compressed = rz.expected(c, keep_len, segments)
    assert want is None or want == stream
    assert r.old_unchanged
    assert r.status == [0] * len(segments), r.status
    assert r.result == [rz.OK, compressed], r.result
    assert r.new_len == len(stream)
    assert r.stream == stream
    assert [int(x) for x in r.new_offs[1:r.new_nb + 2]] == want_offs
    assert (r.out[:PAD] == rz.GUARD).all() and (r.out[PAD + r.new_len:] == rz.GUARD).all()
    assert int(r.new_offs[0]) == GUARD64 and int(r.new_offs[r.new_nb + 2]) == GUARD64
    return r


@pytest.mark.parametrize("name", ["alice", "coding", "terror2", "world192", "xml", "plrabn12"])
def test_gpu_resize_golden_identity(shb, name):
    golden = golden_bytes(name + ".snappy")
    if name == "xml":                                          # (no xml.txt among the goldens: the host decoder's bytes)
        st, plain, _ = shb.decompress_host(golden)
        assert st == 0
    else:
        plain = golden_bytes(name + ".txt")
    g = rc.Container(plain, golden)
    bs, total = g.block_size, g.total
    for cut in (rz.boundary(total, bs, last=False) or total, total // 3, 0):
        r = check_ok(shb, rc.Container(plain[:cut], block_size=bs), cut, [plain[cut:]], want=golden)
        assert r.stream == golden
        assert check_ok(shb, g, cut, []).stream == oracle.compress(plain[:cut], bs)
    x = rz.tail_bytes(plain, total, 777, "random", seed=len(name))
    grown = check_ok(shb, g, total, [x]).stream
    assert check_ok(shb, rc.Container(plain + x, grown), total, [], want=golden).stream == golden


@pytest.mark.parametrize("bs,n", [(1, 200), (7, 1500), (64, 5000), (4096, 30000), (32768, 70000), (65535, 136000)])
def test_gpu_resize_block_sizes_vs_oracle(shb, bs, n):
    """The emulator's cases at its sizes, here every keep_len with every tail at every block size."""
    text = golden_bytes("plrabn12.txt")
    data = datagen.text_random_interleave(text, n, seed=bs)
    c = rc.Container(data, block_size=bs)
    even = rc.Container(data[:n // bs * bs - (bs if bs >= 4096 else 0)], block_size=bs)
    assert even.total % bs == 0 and (bs == 1 or c.total % bs)
    i = 0
    for cont in (c, even):
        for keep_len in rz.keep_lens(cont.total, bs):
            for k in rz.tail_lens(keep_len, bs):
                kind = rz.KINDS[i % 3]
                i += 1
                tail = rz.tail_bytes(cont.plain, keep_len, k, kind, seed=bs + i)
                r = check_ok(shb, cont, keep_len, [tail] if k else [])
                if kind == "same" and k == cont.total - keep_len:
                    assert r.stream == cont.stream


def test_gpu_resize_bulk_form_of_the_parse(shb, monkeypatch):
    """SNAPPY_HIP_K1_STREAM=0: the LDS-table kernel's bulk form, as the product's K1 launch would run it."""
    monkeypatch.setenv("SNAPPY_HIP_K1_STREAM", "0")
    c = rc.Container(golden_bytes("world192.txt")[:300000], block_size=32768)
    check_ok(shb, c, 100000, rz.split(rz.tail_bytes(c.plain, 100000, 250000, "random", seed=1), [70000, 0, 33]))


def test_gpu_resize_header_and_table_size_thresholds(shb):
    text = golden_bytes("plrabn12.txt")
    for small in (127, 16383):
        a = rc.Container(text[:small], block_size=64)
        b = rc.Container(text[:small + 1], block_size=64)
        kept = small // 64
        up = check_ok(shb, a, small, [text[small:small + 1]])
        assert up.stream == b.stream
        assert [int(x) for x in up.new_offs[1:1 + kept]] == [int(x) + 1 for x in a.offsets[:kept]]
        down = check_ok(shb, b, small, [])
        assert down.stream == a.stream
        assert [int(x) for x in down.new_offs[1:1 + kept]] == [int(x) - 1 for x in b.offsets[:kept]]
    for small, large in ((200, 300), (500, 600), (16000, 17000)):
        a = rc.Container(text[:small], block_size=32768)
        b = rc.Container(text[:large], block_size=32768)
        assert check_ok(shb, a, small, [text[small:large]]).stream == b.stream
        assert check_ok(shb, b, small, []).stream == a.stream


def test_gpu_resize_segments_and_empty_ends(shb):
    bs = 64
    text = golden_bytes("terror2.txt")
    c = rc.Container(text[:1000], block_size=bs)
    tail = rz.tail_bytes(c.plain, 990, 150, "random", seed=1)
    pieces = []
    for i, byte in enumerate(tail):
        pieces.append(bytes([byte]))
        if i % 7 == 3:
            pieces.append(b"")
    null_at = pieces.index(b"", 9)
    r = gpu_resize(shb, c, 990, [p if k != null_at else (b"", 0, True) for k, p in enumerate(pieces)])
    assert r.status == [0] * len(pieces) and r.result[0] == rz.OK
    assert r.stream == rz.expected(c, 990, pieces)[0] == check_ok(shb, c, 990, [tail]).stream
    for kind in rz.KINDS:
        tail = rz.tail_bytes(c.plain, 555, sum(rz.mixed_lengths(300, seed=2)), kind, seed=2)
        check_ok(shb, c, 555, rz.split(tail, rz.mixed_lengths(300, seed=2)))
    tail = rz.tail_bytes(c.plain, 1000, 10 + 3 * bs + 9, "zeros")
    check_ok(shb, c, 1000, [tail[:10], tail[10:10 + 3 * bs], tail[10 + 3 * bs:]])
    # empty ends
    e = rc.Container(b"", block_size=4096)
    alice = golden_bytes("alice.txt")
    assert check_ok(shb, e, 0, [alice[:100], alice[100:]]).stream == oracle.compress(alice, 4096)
    assert check_ok(shb, e, 0, []).stream == oracle.compress(b"", 4096)
    k = rc.Container(golden_bytes("coding.txt"), block_size=4096)
    assert check_ok(shb, k, 0, []).stream == oracle.compress(b"", 4096)
    assert check_ok(shb, k, k.total, []).stream == k.stream


def test_gpu_resize_many_more_new_blocks_than_wavefronts(shb):
    """A 64 KiB container at 64-byte blocks with 4 MiB appended in 1,000 segments: 65,536 new blocks (and the one the cut falls
    into), more than the recompress kernel can have wavefronts on a whole MI355X (32 per CU on 256 CUs = 8,192), so that every
    persistent wavefront draws several blocks."""
    bs = 64
    text = golden_bytes("plrabn12.txt")
    c = rc.Container(datagen.text_random_interleave(text, 65536, seed=5), block_size=bs)
    keep_len = 65536 - 17
    tail = datagen.text_random_interleave(text, (4 << 20) + 17, seed=6)
    bounds = np.sort(np.random.default_rng(7).integers(0, len(tail) + 1, 999))
    pieces = [tail[a:b] for a, b in zip([0, *bounds], [*bounds, len(tail)])]
    assert len(pieces) == 1000 and b"".join(pieces) == tail
    new_total = keep_len + len(tail)
    new_nb = shb.num_blocks(new_total, bs)
    compressed = new_nb - keep_len // bs
    # the wavefronts of the recompress kernel, from the scratch's size: every other part of it is known (csrc/snappy_resize.hpp)
    r256 = lambda v: (v + 255) // 256 * 256
    others = 256 + r256((1000 + 1) * 8) + 2 * r256(new_nb * 4) + r256(compressed * 4) + r256(compressed * shb.slot_stride(bs))
    waves, rest = divmod(shb.resize_scratch_bytes(bs, c.num_blocks, new_total, keep_len, 1000) - others, r256(bs + 64))
    assert rest == 0 and 1 <= waves < compressed // 4, (waves, compressed)
    check_ok(shb, c, keep_len, pieces)


def test_gpu_resize_chain_with_an_update_without_host_synchronisation(shb):
    """append, snappy_hip_update_ranges on the result, append, truncate: each call's outputs are the next one's descriptor, with
    an 8-byte device copy of the length between them and nothing read back until the end."""
    import torch
    bs = 4096
    plain0 = golden_bytes("world192.txt")[:500000]
    c = rc.Container(plain0, block_size=bs)
    tail1 = rz.tail_bytes(plain0, len(plain0), 300001, "random", seed=1)
    plain1 = plain0 + tail1
    writes = [(1000, uc.new_bytes(plain1, 1000, 20000, "zeros")), (499990, uc.new_bytes(plain1, 499990, 70000, "random", seed=2))]
    plain2 = uc.patched(plain1, writes)
    tail3 = [golden_bytes("alice.txt"), rz.tail_bytes(plain2, len(plain2), 123457, "random", seed=3)]
    plain3 = plain2 + b"".join(tail3)
    keep4 = 654321
    plain4 = plain3[:keep4]
    totals = [len(plain0), len(plain1), len(plain2), len(plain3), len(plain4)]
    nbs = [shb.num_blocks(t, bs) for t in totals]
    cap = 10 + max(nbs) * shb.slot_stride(bs)
    d_stream = _dev_bytes(c.stream)
    d_off = torch.from_numpy(np.ascontiguousarray(c.offsets, dtype=np.uint64).view(np.int64)).cuda()
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    descs = [shb.make_stream_descs([dict(stream=d_stream, stream_len=len(c.stream), block_offsets=d_off, result=d_res, total_len=c.total,
                                         block_size=bs, header_len=c.header_len, num_blocks=c.num_blocks)])]
    outs, offs, lens, results = [], [], [], []
    for k in range(4):
        outs.append(torch.full((cap,), rz.GUARD, dtype=torch.uint8, device="cuda"))
        offs.append(torch.zeros(nbs[k + 1] + 1, dtype=torch.int64, device="cuda"))
        lens.append(torch.zeros(1, dtype=torch.int64, device="cuda"))
        results.append(torch.full((2,), 0x77, dtype=torch.int32, device="cuda"))
        # the next descriptor: stream_len (the second u64) is filled in on the device
        descs.append(shb.make_stream_descs([dict(stream=outs[k], stream_len=0, block_offsets=offs[k], result=d_res, total_len=totals[k + 1],
                                                 block_size=bs, header_len=0, num_blocks=nbs[k + 1])]))

    def sources(datas):
        d_src = _dev_bytes(b"".join(datas) + b"\0")
        ats = np.concatenate([[0], np.cumsum([len(d) for d in datas])])
        return d_src, [d_src.data_ptr() + int(a) for a in ats[:-1]]

    src1, at1 = sources([tail1])
    src2, at2 = sources([d for _, d in writes])
    src3, at3 = sources(tail3)
    seg1 = shb.make_segments([(at1[0], len(tail1))])
    wr2 = shb.make_writes([(o, len(d), at) for (o, d), at in zip(writes, at2)])
    seg3 = shb.make_segments([(at, len(d)) for at, d in zip(at3, tail3)])
    stats = [torch.full((2,), 0x55, dtype=torch.int32, device="cuda") for _ in range(4)]
    dirty = len(uc.dirty_blocks([(o, len(d)) for o, d in writes], bs))
    scratch = [torch.empty(shb.resize_scratch_bytes(bs, nbs[0], totals[1], totals[0], 1), dtype=torch.uint8, device="cuda"),
               torch.empty(shb.update_scratch_bytes(bs, nbs[1], 2, dirty), dtype=torch.uint8, device="cuda"),
               torch.empty(shb.resize_scratch_bytes(bs, nbs[2], totals[3], totals[2], 2), dtype=torch.uint8, device="cuda"),
               torch.empty(shb.resize_scratch_bytes(bs, nbs[3], totals[4], keep4, 0), dtype=torch.uint8, device="cuda")]
    torch.cuda.synchronize()

    def pass_length(k):
        descs[k + 1].view(torch.int64)[1:2].copy_(lens[k], non_blocking=True)

    # enqueue only: nothing below waits for the device
    shb.resize(descs[0], totals[0], bs, totals[0], totals[1], seg1, 1, stats[0], outs[0], offs[0], lens[0], results[0], d_scratch=scratch[0])
    pass_length(0)
    shb.update_ranges(descs[1], totals[1], bs, wr2, 2, stats[1], outs[1], offs[1], lens[1], results[1], dirty, d_scratch=scratch[1])
    pass_length(1)
    shb.resize(descs[2], totals[2], bs, totals[2], totals[3], seg3, 2, stats[2], outs[2], offs[2], lens[2], results[2], d_scratch=scratch[2])
    pass_length(2)
    shb.resize(descs[3], totals[3], bs, keep4, totals[4], seg3, 0, stats[3], outs[3], offs[3], lens[3], results[3], d_scratch=scratch[3])
    torch.cuda.synchronize()
    assert [int(r.cpu().numpy()[0]) for r in results] == [rz.OK] * 4
    assert [int(x) for x in stats[0].cpu().numpy()[:1]] == [0] and [int(x) for x in stats[1].cpu().numpy()] == [0, 0] \
        and [int(x) for x in stats[2].cpu().numpy()] == [0, 0]
    want = oracle.compress(plain4, bs)
    n = int(lens[3].item())
    assert n == len(want) and bytes(outs[3][:n].cpu().numpy()) == want
    assert [int(x) for x in offs[3].cpu().numpy()] == [int(x) for x in oracle.index_blocks(want)] + [len(want)]
    st, d_back = shb.decompress_resident(outs[3][:n])
    assert st == 0 and bytes(d_back[:len(plain4)].cpu().numpy()) == plain4


def test_gpu_resize_rejected_and_invalid(shb):
    import torch
    text = golden_bytes("terror2.txt")
    for c in (rc.Container(text[:40000], block_size=4096), rc.Container(text[:16384], block_size=4096)):
        for keep_len, segments, new_total, want, capacity in rz.rejected_cases(c):
            r = gpu_resize(shb, c, keep_len, segments, new_total=new_total, capacity=capacity)
            assert r.status == want, (keep_len, r.status)
            assert_untouched(r)
            assert r.result[1] == 0
    c = rc.Container(text[:40000], block_size=4096)
    bs, keep, good = 4096, 10000, [b"abc", b"defgh"]
    assert gpu_resize(shb, c, keep, [(b"", 0, True), b"xyz"]).result[0] == rz.OK
    tail = [rz.tail_bytes(c.plain, keep, 9000, "random", seed=1)]
    need = len(rz.expected(c, keep, tail)[0])
    r = gpu_resize(shb, c, keep, tail, capacity=need - 1)
    assert r.status == [0] and r.result == [rz.REJECTED, rz.expected(c, keep, tail)[2]]
    assert_untouched(r)
    check_ok(shb, c, keep, tail, capacity=need)
    for shape in [(c.total - 1, 4096, c.num_blocks), (c.total, 2048, c.num_blocks), (c.total, 4096, c.num_blocks - 1)]:
        assert_untouched(gpu_resize(shb, c, keep, good, desc_shape=shape))
    # INVALID: a broken link in a kept block, a cut block that does not decode (both damages); OK behind keep_len and on the boundary
    at = int(c.offsets[3])
    broken = bytearray(c.stream)
    broken[at:at + 4] = (int.from_bytes(broken[at:at + 4], "little") - 1).to_bytes(4, "little")
    broken = bytes(broken)
    inside = bytearray(c.stream)
    inside[at + 4] = 0xFF
    inside = bytes(inside)
    tail = [b"the tail"]
    r = gpu_resize(shb, c, 5 * bs + 7, tail, stream=broken)
    assert r.old_unchanged and r.status == [0] and r.result == [rz.INVALID, 1] and r.new_len == 0
    assert gpu_resize(shb, c, 4 * bs, [], stream=broken).result[0] == rz.INVALID
    for stream in (broken, inside):
        r = gpu_resize(shb, c, 3 * bs + 5, tail, stream=stream)
        assert r.old_unchanged and r.result == [rz.INVALID, 1] and r.new_len == 0
        for keep_len in (2 * bs + 100, 3 * bs - 1, 3 * bs, 0):
            check_ok(shb, c, keep_len, tail, stream=stream)
            check_ok(shb, c, keep_len, [], stream=stream)
    r = gpu_resize(shb, c, 6 * bs + 1, tail, stream=inside)
    assert r.result[0] == rz.OK
    assert r.stream[int(r.new_offs[4]):int(r.new_offs[5])] == inside[at:int(c.offsets[4])]
    # host-side argument errors
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d64 = torch.zeros(64, dtype=torch.int64, device="cuda")
    d32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert shb.resize_scratch_bytes(0, 10, 100, 10, 1) == 0 and shb.resize_scratch_bytes(65536, 10, 100, 10, 1) == 0
    with pytest.raises(shb.SnappyHipError):                      # scratch too small
        shb.resize(d, c.total, 4096, 10, 20, d, 1, d32, d, d64, d64, d32, d_scratch=torch.empty(512, dtype=torch.uint8, device="cuda"))
    with pytest.raises(shb.SnappyHipError):                      # scratch misaligned
        shb.resize(d, c.total, 4096, 10, 20, d, 1, d32, d, d64, d64, d32, d_scratch=torch.empty(1 << 20, dtype=torch.uint8, device="cuda")[1:])
    with pytest.raises(shb.SnappyHipError):                      # bad block size
        shb.resize(d, c.total, 65536, 10, 20, d, 1, d32, d, d64, d64, d32, d_scratch=torch.empty(1 << 20, dtype=torch.uint8, device="cuda"))
    with pytest.raises(shb.SnappyHipError):                      # a new length beyond the format's 32 bits
        shb.resize(d, c.total, 4096, 10, 1 << 32, d, 1, d32, d, d64, d64, d32, d_scratch=torch.empty(1 << 20, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()


# ---- drop-in level and CLI: snappy_resize_gpu and dpu_snappy -d -t / -a against the host mode ----

def _cli(args, tmp_path, tag):
    from test_cli import CLI, HOST_DIR
    subprocess.check_call(["make", "-s", "-C", HOST_DIR])
    out = tmp_path / tag
    r = subprocess.run([CLI, *args, "-o", str(out)], capture_output=True, text=True)
    return r, (out.read_bytes() if out.exists() else None)


def test_gpu_dropin_and_cli_resize_match_host_mode(shb, tmp_path):
    path = os.path.join(ROOT, "tests", "golden", "xml.snappy")
    data = open(path, "rb").read()
    st, plain, _ = shb.decompress_host(data)
    assert st == 0
    total, bs = len(plain), 32768
    more = rz.tail_bytes(plain, total, 200001, "random", seed=1)
    cases = [(total // 3, None), (4 * bs, b""), (0, None), (total, b"x"), (total, more), (total // 2, more), (bs - 1, plain[bs - 1:]), (0, b"new")]
    for k, (keep_len, tail) in enumerate(cases):
        want = oracle.compress(plain[:keep_len] + (tail or b""), bs)
        st, got, rt = shb.resize_host(data, keep_len, tail)
        assert st == 0, (keep_len, k)
        assert set(rt) >= {"pre", "d_alloc", "load", "copy_in", "run", "copy_out", "d_free"}
        args = ["-t", str(keep_len)]
        if tail is not None:
            tf = tmp_path / f"tail{k}"
            tf.write_bytes(tail)
            args = (args if keep_len != total else []) + ["-a", str(tf)]
        r_h, host = _cli([*args, "-i", path], tmp_path, f"h{k}")
        r_d, dev = _cli(["-d", *args, "-i", path], tmp_path, f"d{k}")
        assert r_h.returncode == 0 and r_d.returncode == 0, (r_h.stderr, r_d.stderr)
        assert got == want and host == want and dev == want, (keep_len, k)
    # a caller-owned output buffer one byte too small, then exact; keep_len beyond the container; a cut block that does not decode
    want = oracle.compress(plain[:total // 2] + more, bs)
    st, _, _ = shb.resize_host(data, total // 2, more, out_capacity=len(want) - 1)
    assert st == shb.SNAPPY_BUFFER_TOO_SMALL
    st, got, _ = shb.resize_host(data, total // 2, more, out_capacity=len(want))
    assert st == 0 and got == want
    assert shb.resize_host(data, total + 1, b"x")[0] == shb.SNAPPY_INVALID_INPUT
    assert shb.resize_host(data[:-3], 5, b"x")[0] == shb.SNAPPY_INVALID_INPUT             # the chain does not end with the file
    assert shb.resize_host(b"\xff" * 6, 0, b"x")[0] == shb.SNAPPY_INVALID_INPUT
    c = rc.Container(plain, data)
    bad = bytearray(data)
    bad[int(c.offsets[2]) + 4] = 0xFF
    assert shb.resize_host(bytes(bad), 2 * bs + 9, b"x")[0] == shb.SNAPPY_INVALID_INPUT
    st, got, _ = shb.resize_host(bytes(bad), 2 * bs, b"x")                                 # on the boundary it is not decoded
    assert st == 0 and got == oracle.compress(plain[:2 * bs] + b"x", bs)
    r_d, dev = _cli(["-d", "-t", str(total + 1), "-i", path], tmp_path, "beyond.out")
    assert r_d.returncode != 0 and r_d.stderr.strip() and dev is None
