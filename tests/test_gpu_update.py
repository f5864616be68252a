"""GPU tests (-m gpu) of the container update through the C ABI (snappy_hip_update_ranges): the matrix of
tests/test_update_emulated.py on the device at larger sizes, a 1 GiB Silesia-mix container with ~10k writes, chained updates
without host synchronisation, the drop-in call and the CLI, and the generated code.  The check is an identity with no
tolerance: the new stream == oracle.compress(plaintext with the writes applied)."""
import os
import re
import subprocess

import numpy as np
import pytest

import container_cases as cc
import datagen
import oracle_lib as oracle
import ranges_cases as rc
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


def gpu_update(shb, c, writes, max_dirty=None, capacity=None, stream=None, desc_shape=None):
    """As test_update_emulated.run, on the device.  writes: list of (offset, data) or (offset, data, length, null src)."""
    import torch
    nb = c.num_blocks
    old = c.stream if stream is None else stream
    d_stream = _dev_bytes(old)
    d_off = torch.from_numpy(np.ascontiguousarray(c.offsets if nb else np.zeros(1), dtype=np.uint64).view(np.int64)).cuda()
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    dt, dbs, dnb = desc_shape or (c.total, c.block_size, nb)
    d_desc = shb.make_stream_descs([dict(stream=d_stream, stream_len=len(old), block_offsets=d_off, result=d_res, total_len=dt,
                                         block_size=dbs, header_len=c.header_len, num_blocks=dnb)])
    # the sources packed into one buffer, every one behind i % 16 + 1 spare bytes (all alignments)
    packed, entries = bytearray(), []
    for i, w in enumerate(writes):
        off, data = w[0], w[1]
        length = w[2] if len(w) > 2 else len(data)
        null = w[3] if len(w) > 3 else False
        packed += bytes(i % 16 + 1)
        entries.append((off, length, None if null else len(packed)))
        packed += data
    d_src = _dev_bytes(bytes(packed) + b"\0")
    d_writes = shb.make_writes([(o, n, 0 if at is None else d_src.data_ptr() + at) for o, n, at in entries])
    if max_dirty is None:
        max_dirty = max(nb, 1)
    if capacity is None:
        capacity = 10 + nb * shb.slot_stride(c.block_size)
    out = torch.full((capacity + 2 * PAD,), uc.GUARD, dtype=torch.uint8, device="cuda")
    new_offs = torch.from_numpy(np.full(nb + 3, GUARD64, dtype=np.uint64).view(np.int64)).cuda()
    new_len = torch.from_numpy(np.full(1, GUARD64, dtype=np.uint64).view(np.int64)).cuda()
    result = torch.full((2,), 0x77, dtype=torch.int32, device="cuda")
    status = torch.full((max(len(writes), 1),), 0x55, dtype=torch.int32, device="cuda")
    shb.update_ranges(d_desc, c.total, c.block_size, d_writes, len(writes), status, out[PAD:], new_offs[1:], new_len, result, max_dirty,
                      capacity=capacity)
    torch.cuda.synchronize()
    r = Result()
    r.old_unchanged = bytes(d_stream.cpu().numpy()[:len(old)]) == old
    r.status = [int(x) for x in status.cpu().numpy()[:len(writes)]]
    r.result = [int(x) for x in result.cpu().numpy()]
    r.new_len = int(new_len.cpu().numpy().view(np.uint64)[0])
    r.out = out.cpu().numpy()
    r.new_offs = new_offs.cpu().numpy().view(np.uint64)
    return r


def assert_untouched(r):
    assert r.old_unchanged
    assert r.result[0] == uc.REJECTED
    assert r.new_len == 0
    assert (r.out == uc.GUARD).all()
    assert (r.new_offs == GUARD64).all()


def check_ok(shb, c, writes, **kw):
    r = gpu_update(shb, c, writes, **kw)
    want, want_offs, dirty = uc.expected(c, writes)
    assert r.old_unchanged
    assert r.status == [0] * len(writes), r.status
    assert r.result == [uc.OK, dirty], r.result
    assert r.new_len == len(want)
    assert r.out[PAD:PAD + r.new_len].tobytes() == want
    assert [int(x) for x in r.new_offs[1:c.num_blocks + 2]] == want_offs
    assert (r.out[:PAD] == uc.GUARD).all() and (r.out[PAD + r.new_len:] == uc.GUARD).all()
    assert int(r.new_offs[0]) == GUARD64 and int(r.new_offs[c.num_blocks + 2]) == GUARD64
    return r


def with_data(c, ranges, kind, seed=0):
    return [(o, uc.new_bytes(c.plain, o, n, kind, seed)) for o, n in ranges]


@pytest.mark.parametrize("name", ["alice", "coding", "terror2", "plrabn12", "world192"])
def test_gpu_update_goldens(shb, name):
    c = rc.Container(golden_bytes(name + ".txt"), golden_bytes(name + ".snappy"))
    sets = uc.write_sets(c.total, c.block_size, seed=len(name), random_count=12)
    for i, ws in enumerate(sets):
        for kind in (uc.KINDS if len(ws) > 1 else (uc.KINDS[i % 3],)):
            r = check_ok(shb, c, with_data(c, ws, kind, seed=i))
            if kind == "same":
                assert r.out[PAD:PAD + r.new_len].tobytes() == c.stream


# (64, 65600): 1025 blocks, one more than a trip of the planners' loops (the write of the whole container dirties every one)
@pytest.mark.parametrize("bs,n", [(1, 3000), (7, 20000), (64, 65600), (64, 200000), (4096, 1000000), (32768, 3000000), (65535, 3000000)])
@pytest.mark.parametrize("kind", uc.KINDS)
def test_gpu_update_block_sizes_vs_oracle(shb, bs, n, kind):
    text = golden_bytes("plrabn12.txt")
    c = rc.Container(datagen.text_random_interleave(text, n, seed=bs), block_size=bs)
    nb = c.num_blocks
    last = (nb - 1) * bs
    ranges = uc.disjoint([(b * bs - 1, 1) for b in (1, nb // 2, nb - 1) if 0 < b < nb] + [(b * bs, 1) for b in (1, nb - 1) if 0 < b < nb] +
                         [(max(last - 3, 0), c.total - max(last - 3, 0))])
    check_ok(shb, c, with_data(c, ranges, kind, seed=bs))
    check_ok(shb, c, with_data(c, [(0, c.total)], kind, seed=bs + 1))
    for ws in uc.write_sets(c.total, bs, seed=bs, random_count=40)[-3:]:
        check_ok(shb, c, with_data(c, ws, kind, seed=bs + 3))


def test_gpu_update_bulk_form_of_the_parse(shb, monkeypatch):
    """SNAPPY_HIP_K1_STREAM=0: the LDS-table kernel's bulk form, as the product's K1 launch would run it."""
    monkeypatch.setenv("SNAPPY_HIP_K1_STREAM", "0")
    c = rc.Container(golden_bytes("world192.txt"), block_size=32768)
    check_ok(shb, c, with_data(c, uc.write_sets(c.total, 32768, seed=3, random_count=20)[-3], "random", seed=1))


def test_gpu_update_no_writes_empty_writes_empty_container(shb):
    c = rc.Container(golden_bytes("world192.txt"), golden_bytes("world192.snappy"))
    r = check_ok(shb, c, [])
    assert r.out[PAD:PAD + r.new_len].tobytes() == c.stream
    r = check_ok(shb, c, [(0, b""), (5, b""), (c.block_size, b""), (c.total, b""), (c.total, b"")])
    assert r.out[PAD:PAD + r.new_len].tobytes() == c.stream
    check_ok(shb, c, [(5, b""), (5, b"xyz"), (8, b""), (c.total, b"")], max_dirty=1)
    e = rc.Container(b"", block_size=32768)
    r = check_ok(shb, e, [])
    assert r.out[PAD:PAD + r.new_len].tobytes() == oracle.compress(b"", 32768)
    check_ok(shb, e, [(0, b"")])


def test_gpu_update_rejected_and_invalid(shb):
    import torch
    c = rc.Container(golden_bytes("terror2.txt"), block_size=4096)
    big = (1 << 64) - 1
    good = [(10, b"abc"), (5000, b"defgh")]
    cases = [
        ([(c.total - 2, b"xyz")], [uc.OUT_OF_BOUNDS]),
        ([(c.total + 1, b"")], [uc.OUT_OF_BOUNDS]),
        ([(big - 1, b"xy", 5, False)], [uc.OUT_OF_BOUNDS]),
        ([(7, b"", big, False)], [uc.OUT_OF_BOUNDS]),
        ([(7, b"", 3, True)], [uc.OUT_OF_BOUNDS]),
        ([(100, b"abc"), (50, b"de")], [0, uc.UNORDERED]),
        ([(100, b"abcd"), (103, b"de")], [0, uc.UNORDERED]),
        (good + [(c.total - 2, b"xyz")], [0, 0, uc.OUT_OF_BOUNDS]),
        ([good[0], (4, b"z"), good[1]], [0, uc.UNORDERED, 0]),
        ([good[0], (20, b"", 3, True), (21, b"q"), good[1]], [0, uc.OUT_OF_BOUNDS, uc.UNORDERED, 0]),
        ([(big - 1, b"xy", 5, False), (9, b"a")], [uc.OUT_OF_BOUNDS, uc.UNORDERED]),
    ]
    for writes, want in cases:
        r = gpu_update(shb, c, writes)
        assert r.status == want, (writes, r.status)
        assert_untouched(r)
    # one dirty block too many; capacity one byte short; a descriptor of another shape
    writes = [(4095, b"ab"), (20000, b"c")]
    r = gpu_update(shb, c, writes, max_dirty=2)
    assert r.status == [0, 0] and r.result == [uc.REJECTED, 3]
    assert_untouched(r)
    check_ok(shb, c, writes, max_dirty=3)
    writes = with_data(c, [(100, 9000)], "random", seed=1)
    need = len(uc.expected(c, writes)[0])
    assert_untouched(gpu_update(shb, c, writes, capacity=need - 1))
    check_ok(shb, c, writes, capacity=need)
    for shape in [(c.total - 1, 4096, c.num_blocks), (c.total, 2048, c.num_blocks), (c.total, 4096, c.num_blocks - 1)]:
        assert_untouched(gpu_update(shb, c, [(10, b"abc")], desc_shape=shape))
    # INVALID: a broken link at a clean block, a damaged dirty block partly overwritten; OK when it is overwritten completely
    bs = 4096
    at = int(c.offsets[3])
    broken = bytearray(c.stream)
    broken[at:at + 4] = (int.from_bytes(broken[at:at + 4], "little") - 1).to_bytes(4, "little")
    broken = bytes(broken)
    inside = bytearray(c.stream)
    inside[at + 4] = 0xFF
    inside = bytes(inside)
    for stream, writes in ((broken, [(10, b"abc")]), (broken, []), (broken, [(3 * bs + 5, b"abc")]), (inside, [(3 * bs + 5, b"abc")])):
        r = gpu_update(shb, c, writes, stream=stream)
        assert r.old_unchanged and r.result[0] == uc.INVALID and r.new_len == 0, (writes, r.result)
    for stream in (broken, inside):
        check_ok(shb, c, with_data(c, [(3 * bs, bs)], "random", seed=5), stream=stream)
        check_ok(shb, c, with_data(c, [(3 * bs - 7, 100), (3 * bs + 93, bs)], "zeros"), stream=stream)
    r = gpu_update(shb, c, [(10, b"abc")], stream=inside)
    assert r.result[0] == uc.OK
    assert r.out[PAD:PAD + r.new_len].tobytes()[int(r.new_offs[4]):int(r.new_offs[5])] == inside[at:int(c.offsets[4])]
    # host-side argument errors
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d64 = torch.zeros(64, dtype=torch.int64, device="cuda")
    d32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert shb.update_scratch_bytes(0, 10, 1, 1) == 0
    with pytest.raises(shb.SnappyHipError):                      # scratch too small
        shb.update_ranges(d, c.total, 4096, d, 1, d32, d, d64, d64, d32, 4, d_scratch=torch.empty(512, dtype=torch.uint8, device="cuda"))
    with pytest.raises(shb.SnappyHipError):                      # no dirty block allowed, but a write
        shb.update_ranges(d, c.total, 4096, d, 1, d32, d, d64, d64, d32, 0)
    with pytest.raises(shb.SnappyHipError):                      # bad block size
        shb.update_ranges(d, c.total, 65536, d, 1, d32, d, d64, d64, d32, 4, d_scratch=torch.empty(1 << 20, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()


def _resident(shb, d_stream):
    """Descriptor of a resident stream, indexed on the device -> (desc tensor, total, bs, nb, tensors to keep)."""
    import torch
    total, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
    nb = shb.num_blocks(total, bs)
    d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_desc = shb.make_stream_descs([dict(stream=d_stream, stream_len=d_stream.numel(), block_offsets=d_boff, result=d_res, total_len=total,
                                         block_size=bs, header_len=hdr, num_blocks=nb)])
    shb.index_streams(d_desc, 1)
    return d_desc, total, bs, nb, [d_boff, d_res]


def test_gpu_update_three_chained_updates_without_host_synchronisation(shb):
    import torch
    plain = golden_bytes("world192.txt")
    bs = 4096
    c = rc.Container(plain, block_size=bs)
    nb = c.num_blocks
    rounds = [with_data(c, uc.disjoint([(1000, 20000), (300000, 5), (700000, 123456)]), "random", seed=1),
              with_data(c, uc.disjoint([(0, 4096), (15000, 40000), (1100000, c.total - 1100000)]), "zeros"),
              with_data(c, uc.disjoint([(4095, 2), (20000, 300000), (900000, 1)]), "random", seed=3)]
    final = plain
    for ws in rounds:
        final = uc.patched(final, ws)
    cap = 10 + nb * shb.slot_stride(bs)
    d_stream = _dev_bytes(c.stream)
    d_off = torch.from_numpy(np.ascontiguousarray(c.offsets, dtype=np.uint64).view(np.int64)).cuda()
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    descs = [shb.make_stream_descs([dict(stream=d_stream, stream_len=len(c.stream), block_offsets=d_off, result=d_res, total_len=c.total,
                                         block_size=bs, header_len=c.header_len, num_blocks=nb)])]
    outs, offs, lens, results, keep = [], [], [], [], []
    for k in range(3):
        outs.append(torch.full((cap,), uc.GUARD, dtype=torch.uint8, device="cuda"))
        offs.append(torch.zeros(nb + 1, dtype=torch.int64, device="cuda"))
        lens.append(torch.zeros(1, dtype=torch.int64, device="cuda"))
        results.append(torch.full((2,), 0x77, dtype=torch.int32, device="cuda"))
        # the next descriptor: stream_len (the second u64) is filled in on the device
        descs.append(shb.make_stream_descs([dict(stream=outs[k], stream_len=0, block_offsets=offs[k], result=d_res, total_len=c.total,
                                                 block_size=bs, header_len=c.header_len, num_blocks=nb)]))
    prepared = []
    for ws in rounds:
        packed = b"".join(d for _, d in ws)
        d_src = _dev_bytes(packed)
        at, entries = 0, []
        for o, d in ws:
            entries.append((o, len(d), d_src.data_ptr() + at))
            at += len(d)
        prepared.append((shb.make_writes(entries), len(ws), torch.zeros(len(ws), dtype=torch.int32, device="cuda"), d_src))
    scratch = torch.empty(shb.update_scratch_bytes(bs, nb, 3, nb), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k in range(3):                                           # enqueue only: nothing below waits for the device
        d_writes, count, d_status, _ = prepared[k]
        shb.update_ranges(descs[k], c.total, bs, d_writes, count, d_status, outs[k], offs[k], lens[k], results[k], nb, d_scratch=scratch)
        descs[k + 1].view(torch.int64)[1:2].copy_(lens[k], non_blocking=True)
    torch.cuda.synchronize()
    for k in range(3):
        assert [int(x) for x in results[k].cpu().numpy()][0] == uc.OK
        assert int((prepared[k][2] != 0).sum().item()) == 0
    want = oracle.compress(final, bs)
    n = int(lens[2].item())
    assert n == len(want) and bytes(outs[2][:n].cpu().numpy()) == want
    assert [int(x) for x in offs[2].cpu().numpy()] == [int(x) for x in oracle.index_blocks(want)] + [len(want)]


def test_gpu_update_silesia_mix_1gib_10k_writes(shb):
    """A resident 1 GiB Silesia-mix container, ~10k seeded sorted writes of 1 B .. 1 MiB (log-uniform, random bytes and
    zeros), against oracle.compress of the patched plaintext (16 threads), and decoded back on the device."""
    import torch
    import silesia_mix
    st, d_xml = shb.decompress_resident(_dev_bytes(golden_bytes("xml.snappy")))
    assert st == 0
    unit = silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0)
    n = 1 << 30
    d_in = silesia_mix.container_from_unit(torch.from_numpy(unit.copy()).cuda(), n)
    d_stream = shb.compress_resident(d_in, 32768, n=n)
    d_desc, total, bs, nb, keep = _resident(shb, d_stream)
    assert total == n
    rng = np.random.default_rng(77)
    count = 10_000
    lengths = np.clip(np.exp(rng.uniform(0.0, np.log(float(1 << 20)), count)).astype(np.int64), 1, 1 << 20)
    offsets = (rng.random(count) * (total - lengths + 1)).astype(np.int64)
    ranges = uc.disjoint([(int(o), int(k)) for o, k in zip(offsets, lengths)])
    src_off = np.concatenate([[0], np.cumsum([k for _, k in ranges])]).astype(np.int64)
    src = rng.integers(0, 256, int(src_off[-1]) + 1, dtype=np.uint8)
    for i, (o, k) in enumerate(ranges):                          # every third write brings zeros: blocks shrink as well as grow
        if i % 3 == 0:
            src[src_off[i]:src_off[i] + k] = 0
    d_src = torch.from_numpy(src).cuda()
    d_writes = shb.make_writes([(o, k, d_src.data_ptr() + int(src_off[i])) for i, (o, k) in enumerate(ranges)])
    dirty = len(uc.dirty_blocks(ranges, bs))
    plain = d_in[:n].cpu().numpy()
    del d_in
    for i, (o, k) in enumerate(ranges):
        plain[o:o + k] = src[src_off[i]:src_off[i] + k]
    want = oracle.compress(plain, bs, threads=16)
    cap = d_stream.numel() + dirty * shb.slot_stride(bs)
    d_new = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_noff = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_result = torch.full((2,), 0x77, dtype=torch.int32, device="cuda")
    d_status = torch.full((len(ranges),), 0x55, dtype=torch.int32, device="cuda")
    shb.update_ranges(d_desc, total, bs, d_writes, len(ranges), d_status, d_new, d_noff, d_len, d_result, dirty)
    torch.cuda.synchronize()
    assert [int(x) for x in d_result.cpu().numpy()] == [uc.OK, dirty]
    assert int((d_status != 0).sum().item()) == 0
    new_len = int(d_len.item())
    assert new_len == len(want)
    assert torch.equal(d_new[:new_len].cpu(), torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()))
    assert [int(x) for x in d_noff.cpu().numpy()[[0, 1, nb // 2, nb]]] == \
        [int(x) for x in np.concatenate([oracle.index_blocks(want), [len(want)]])[[0, 1, nb // 2, nb]]]
    st, d_back = shb.decompress_resident(d_new[:new_len])
    assert st == 0 and torch.equal(d_back[:n].cpu(), torch.from_numpy(plain))


def test_update_kernels_use_global_not_flat_instructions(tmp_path):
    """The recompress kernel runs K2's decoder and K1's parse, which rely on global_* operations of one wavefront completing
    in issue order (tests/test_abi_symbols.py); its pointers come from descriptors in memory, so the check is repeated on the
    code of every update kernel."""
    import __graft_entry__ as entry
    src = os.path.join(ROOT, "pim-compression_amd", "csrc", "snappy_hip.hip")
    asm = tmp_path / "device.s"
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(asm)])
    text = asm.read_text()
    for name, least in (("update_mark_kernel", 3), ("update_plan_kernel", 3), ("recompress_dirty_kernelILi2E", 20),
                        ("recompress_dirty_kernelILi3E", 20), ("update_sizes_kernel", 3), ("merge_stream_kernel", 3)):
        m = re.search(r"^(_ZN10snappy_hip\d+" + name + r"\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
        assert m, name
        assert re.findall(r"^\s*flat_\w+", m.group(2), re.M) == [], name
        assert len(re.findall(r"^\s*global_(?:load|store|atomic)", m.group(2), re.M)) >= least, name


# ---- drop-in level and CLI: snappy_update_range_gpu and dpu_snappy -d -w against host-mode -w ----

def _cli_update(args, tmp_path, tag):
    from test_cli import CLI, HOST_DIR
    subprocess.check_call(["make", "-s", "-C", HOST_DIR])
    out = tmp_path / tag
    r = subprocess.run([CLI, *args, "-o", str(out)], capture_output=True, text=True)
    return r, (out.read_bytes() if out.exists() else None)


def test_gpu_dropin_and_cli_update_match_host_mode(shb, tmp_path):
    path = os.path.join(ROOT, "tests", "golden", "xml.snappy")
    data = open(path, "rb").read()
    st, plain, _ = shb.decompress_host(data)
    assert st == 0
    total = len(plain)
    rng = np.random.default_rng(85)
    cases = [(0, 1), (32767, 2), (total - 1, 1), (0, total), (12345, 0), (32768, 32768)]
    cases += [(int(o), int(min(total - o, n))) for o, n in zip(rng.integers(0, total, 3), rng.integers(1, 1 << 20, 3))]
    for k, (off, n) in enumerate(cases):
        patch = uc.new_bytes(plain, off, n, uc.KINDS[k % 3], seed=k)
        want = oracle.compress(uc.patched(plain, [(off, patch)]), 32768)
        st, got, rt = shb.update_range_host(data, off, patch)
        assert st == 0, (off, n)
        assert set(rt) >= {"pre", "d_alloc", "load", "copy_in", "run", "copy_out", "d_free"}
        pf = tmp_path / f"patch{k}"
        pf.write_bytes(patch)
        r_h, host = _cli_update(["-w", f"{off}:{pf}", "-i", path], tmp_path, f"h{k}")
        r_d, dev = _cli_update(["-d", "-w", f"{off}:{pf}", "-i", path], tmp_path, f"d{k}")
        assert r_h.returncode == 0 and r_d.returncode == 0, (r_h.stderr, r_d.stderr)
        assert got == want and host == want and dev == want, (off, n)
    # a caller-owned output buffer too small for the new stream; a patch beyond the container
    patch = bytes(100)
    want = oracle.compress(uc.patched(plain, [(10, patch)]), 32768)
    st, _, _ = shb.update_range_host(data, 10, patch, out_capacity=len(want) - 1)
    assert st == shb.SNAPPY_BUFFER_TOO_SMALL
    st, got, _ = shb.update_range_host(data, 10, patch, out_capacity=len(want))
    assert st == 0 and got == want
    st, _, _ = shb.update_range_host(data, total - 50, patch)
    assert st == shb.SNAPPY_INVALID_INPUT
    pf = tmp_path / "beyond"
    pf.write_bytes(patch)
    r_d, dev = _cli_update(["-d", "-w", f"{total - 50}:{pf}", "-i", path], tmp_path, "beyond.out")
    assert r_d.returncode != 0 and r_d.stderr.strip() and dev is None
    # coding.txt at 1000-byte blocks, a write through blocks 2..4: each damaged variant gets the status that the front end's CPU
    # test (tests/test_dropin_plan.py) holds to the model -- an update walks the whole chain, so only the intact one passes
    plain = golden_bytes("coding.txt")
    stream = oracle.compress(plain, 1000)
    off, n = cc.inner_span(1000)
    patch = uc.new_bytes(plain, off, n, "random", seed=9)
    want = oracle.compress(uc.patched(plain, [(off, patch)]), 1000)
    for kind, bad in cc.damaged(stream).items():
        st, got, _ = shb.update_range_host(bad, off, patch)
        assert st == cc.model(bad, off, n, update=True)[0] == (0 if kind == "intact" else shb.SNAPPY_INVALID_INPUT), kind
        assert got == (want if st == 0 else b""), kind
    st, _, _ = shb.update_range_host(stream, off, patch, out_capacity=len(want) - 1)
    assert st == shb.SNAPPY_BUFFER_TOO_SMALL
    st, got, _ = shb.update_range_host(stream, off, patch, out_capacity=len(want))
    assert st == 0 and got == want
