"""GPU tests (-m gpu) of the range decoder through the C ABI (snappy_hip_decompress_ranges): the matrix of
tests/test_ranges_emulated.py on the device, a 1 GiB Silesia-mix container with 100k ranges, and the generated code."""
import os
import re
import subprocess

import numpy as np
import pytest

import container_cases as cc
import datagen
import oracle_lib as oracle
import ranges_cases as rc
from conftest import golden_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def gpu_descs(shb, containers, streams=None):
    """Device copies of the streams + their block offsets -> (descs tensor, tensors to keep alive)."""
    import torch
    keep, entries = [], []
    for i, c in enumerate(containers):
        d_stream = _dev_bytes(c.stream if streams is None else streams[i])
        d_off = torch.from_numpy(np.ascontiguousarray(c.offsets if c.num_blocks else np.zeros(1), dtype=np.uint64).view(np.int64)).cuda()
        d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
        keep += [d_stream, d_off, d_res]
        entries.append(dict(stream=d_stream, stream_len=d_stream.numel(), block_offsets=d_off, result=d_res, total_len=c.total,
                            block_size=c.block_size, header_len=c.header_len, num_blocks=c.num_blocks))
    return shb.make_stream_descs(entries), keep


def gpu_run(shb, containers, requests, dst_offsets=None, buf_len=None, slots=None, max_block_size=None, streams=None):
    """As test_ranges_emulated.run, on the device: (statuses, destination buffer as numpy, dst offsets)."""
    import torch
    descs, keep = gpu_descs(shb, containers, streams)
    if dst_offsets is None:
        dst_offsets, buf_len = rc.layout([int(n) if n < (1 << 40) else 0 for _, _, n in requests])
    buf = torch.full((buf_len,), rc.GUARD, dtype=torch.uint8, device="cuda")
    d_ranges = shb.make_ranges([(s, off, n, buf.data_ptr() + dst_offsets[i]) for i, (s, off, n) in enumerate(requests)])
    d_status = torch.full((len(requests),), 0x55, dtype=torch.int32, device="cuda")
    mbs = max_block_size or max(c.block_size for c in containers)
    scratch = None
    if slots is not None:
        prefix = ((len(requests) + 2) * 8 + 255) & ~255
        scratch = torch.empty(prefix + slots * ((mbs + 255) & ~255), dtype=torch.uint8, device="cuda")
    shb.decompress_ranges(descs, len(containers), d_ranges, len(requests), d_status, mbs, scratch)
    torch.cuda.synchronize()
    return [int(x) for x in d_status.cpu().numpy()], buf.cpu().numpy(), dst_offsets


def check_ok(shb, containers, requests, **kw):
    st, buf, offs = gpu_run(shb, containers, requests, **kw)
    assert st == [0] * len(requests), [(requests[i], x) for i, x in enumerate(st) if x != 0]
    assert rc.check_buffer(buf, [(offs[i], n, containers[s].plain[o:o + n]) for i, (s, o, n) in enumerate(requests)]) == []


@pytest.mark.parametrize("name", ["alice", "coding", "terror2", "plrabn12", "world192"])
def test_gpu_ranges_goldens(shb, name):
    c = rc.Container(golden_bytes(name + ".txt"), golden_bytes(name + ".snappy"))
    check_ok(shb, [c], [(0, o, n) for o, n in rc.boundary_ranges(c.total, c.block_size, seed=len(name), random_count=200)])


@pytest.mark.parametrize("bs,n", [(1, 3000), (7, 20000), (64, 200000), (4096, 1000000), (32768, 3000000), (65535, 3000000)])
def test_gpu_ranges_block_sizes_vs_oracle(shb, bs, n):
    text = golden_bytes("plrabn12.txt")
    c = rc.Container(datagen.text_random_interleave(text, n, seed=bs), block_size=bs)
    check_ok(shb, [c], [(0, o, k) for o, k in rc.boundary_ranges(c.total, bs, seed=bs, random_count=300)])


def test_gpu_ranges_mixed_block_sizes_overlaps_and_one_slot(shb):
    text = golden_bytes("plrabn12.txt")
    cs = [rc.Container(text[:700], block_size=7), rc.Container(text[:200000], block_size=4096), rc.Container(text, block_size=65535),
          rc.Container(datagen.periodic(30000, 13), block_size=64), rc.Container(golden_bytes("world192.txt"), block_size=32768)]
    reqs = []
    for i, c in enumerate(cs):
        reqs += [(i, o, n) for o, n in rc.boundary_ranges(c.total, c.block_size, seed=i, random_count=30)]
    reqs += [(1, 1000, 9000), (1, 1000, 9000), (4, 0, cs[4].total), (4, 0, cs[4].total)]       # overlapping ranges
    check_ok(shb, cs, reqs)
    check_ok(shb, cs, reqs, slots=1)


def test_gpu_ranges_adjacent_rebuild_the_plaintext(shb):
    c = rc.Container(golden_bytes("world192.txt"), block_size=4096)
    rng = np.random.default_rng(5)
    cuts = sorted({0, c.total} | {int(x) for x in rng.integers(0, c.total, 400)} | {4096, 4097, 8191})
    reqs = [(0, a, b - a) for a, b in zip(cuts, cuts[1:])]
    st, buf, _ = gpu_run(shb, [c], reqs, dst_offsets=[29 + a for a, _ in zip(cuts, cuts[1:])], buf_len=29 + c.total + 31)
    assert st == [0] * len(reqs)
    assert rc.check_buffer(buf, [(29, c.total, c.plain)]) == []


def test_gpu_ranges_one_more_than_a_planner_trip(shb):
    """range_pieces_kernel takes 1024 ranges per trip of its loop: 1025 ranges over a 64 KiB container, so the last range's
    pieces start at the carry of the first trip.  Ranges of no pieces (length 0) sit among the others."""
    c = rc.Container(golden_bytes("world192.txt")[:65536], block_size=4096)
    rng = np.random.default_rng(1025)
    reqs = [(0, int(o), int(min(c.total - o, n)) * (i % 5 != 0)) for i, (o, n) in enumerate(zip(rng.integers(0, c.total, 1025), rng.integers(1, 9000, 1025)))]
    assert len(reqs) == 1025 and reqs[1024][2] > 0
    check_ok(shb, [c], reqs)


def test_gpu_ranges_out_of_bounds_damage_and_arguments(shb):
    import torch
    c = rc.Container(golden_bytes("terror2.txt"), block_size=4096)
    big = (1 << 64) - 1
    reqs = [(0, c.total - 10, 11), (0, c.total + 1, 0), (0, big, 2), (0, 5, big), (1, 0, 10), (7, 0, 0), (0, 100, 50)]
    st, buf, offs = gpu_run(shb, [c], reqs, dst_offsets=[40 * i + 7 for i in range(len(reqs))], buf_len=40 * len(reqs) + 64)
    assert st == [rc.OUT_OF_BOUNDS] * 6 + [0]
    assert rc.check_buffer(buf, [(offs[6], 50, c.plain[100:150])]) == []
    # one damaged block: the ranges that touch it are INVALID, the others exact
    damaged = bytearray(c.stream)
    at = int(c.offsets[3])
    damaged[at:at + 4] = (int.from_bytes(damaged[at:at + 4], "little") - 1).to_bytes(4, "little")
    bs = c.block_size
    reqs = [(0, 3 * bs + 10, 5), (0, 2 * bs, 2 * bs), (0, 0, 3 * bs), (0, 4 * bs, 3 * bs), (0, 3 * bs - 1, 1), (0, 4 * bs, 1),
            (0, 0, c.total), (0, 3 * bs, bs)]
    touched = [True, True, False, False, False, False, True, True]
    st, buf, offs = gpu_run(shb, [c], reqs, streams=[bytes(damaged)])
    assert st == [1 if t else 0 for t in touched], st
    assert rc.check_buffer(buf, [(offs[i], n, "any" if touched[i] else c.plain[o:o + n]) for i, (_, o, n) in enumerate(reqs)]) == []
    # arguments: scratch query, a scratch too small for one slot, a bad max_block_size
    assert shb.decompress_ranges_scratch_bytes(0, 10) == 0
    assert shb.decompress_ranges_scratch_bytes(32768, 10) >= 256 + 32768
    descs, keep = gpu_descs(shb, [c])
    d_ranges = shb.make_ranges([(0, 0, 10, keep[0].data_ptr())])
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(shb.SnappyHipError):
        shb.decompress_ranges(descs, 1, d_ranges, 1, d_status, 4096, torch.empty(256 + 4095, dtype=torch.uint8, device="cuda"))
    with pytest.raises(shb.SnappyHipError):
        shb.decompress_ranges(descs, 1, d_ranges, 1, d_status, 65536)


def test_gpu_ranges_silesia_mix_1gib_100k_ranges(shb):
    """A resident 1 GiB Silesia-mix container, 100k seeded ranges of 1 B .. 1 MiB (log-uniform) packed into one buffer behind
    guard gaps, against a full decode of the same stream."""
    import torch
    import silesia_mix
    st, d_xml = shb.decompress_resident(_dev_bytes(golden_bytes("xml.snappy")))
    assert st == 0
    unit = silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0)
    n = 1 << 30
    d_in = silesia_mix.container_from_unit(torch.from_numpy(unit.copy()).cuda(), n)
    d_stream = shb.compress_resident(d_in, 32768, n=n)
    st, d_full = shb.decompress_resident(d_stream)
    assert st == 0 and torch.equal(d_full[:n], d_in[:n])
    del d_in
    total, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
    nb = shb.num_blocks(total, bs)
    d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    descs = shb.make_stream_descs([dict(stream=d_stream, stream_len=d_stream.numel(), block_offsets=d_boff, result=d_res, total_len=total,
                                        block_size=bs, header_len=hdr, num_blocks=nb)])
    shb.index_streams(descs, 1)
    rng = np.random.default_rng(2024)
    count = 100_000
    lengths = np.exp(rng.uniform(0.0, np.log(float(1 << 20)), count)).astype(np.int64)
    lengths = np.clip(lengths, 1, 1 << 20)
    offsets = (rng.random(count) * (total - lengths + 1)).astype(np.int64)
    gap = 16
    dst = np.cumsum(lengths + gap) - lengths                                # range i at dst[i], gap bytes in front of it
    buf_len = int(dst[-1] + lengths[-1] + gap)
    buf = torch.full((buf_len,), rc.GUARD, dtype=torch.uint8, device="cuda")
    d_ranges = shb.make_ranges([(0, int(o), int(k), buf.data_ptr() + int(d)) for o, k, d in zip(offsets, lengths, dst)])
    d_status = torch.full((count,), 0x55, dtype=torch.int32, device="cuda")
    shb.decompress_ranges(descs, 1, d_ranges, count, d_status, bs)
    torch.cuda.synchronize()
    assert int((d_status != 0).sum().item()) == 0
    bad = [i for i in range(count) if not torch.equal(buf[int(dst[i]):int(dst[i] + lengths[i])], d_full[int(offsets[i]):int(offsets[i] + lengths[i])])]
    assert bad == [], bad[:10]
    gaps = torch.from_numpy((dst[:, None] - gap + np.arange(gap)[None, :]).reshape(-1)).cuda()
    assert bool((buf[gaps] == rc.GUARD).all().item())
    assert bool((buf[buf_len - gap:] == rc.GUARD).all().item())


def test_range_kernels_use_global_not_flat_instructions(tmp_path):
    """The range kernel runs K2's decoder, which relies on global_* operations of one wavefront completing in issue order
    (tests/test_abi_symbols.py); its pointers come from descriptors in memory, so the check is repeated on its code."""
    import __graft_entry__ as entry
    src = os.path.join(ROOT, "pim-compression_amd", "csrc", "snappy_hip.hip")
    asm = tmp_path / "device.s"
    subprocess.check_call([entry.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(asm)])
    text = asm.read_text()
    for name in ("decompress_ranges_kernel", "range_pieces_kernel"):
        m = re.search(r"^(_ZN10snappy_hip\d+" + name + r"\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
        assert m, name
        assert re.findall(r"^\s*flat_\w+", m.group(2), re.M) == [], name
        assert len(re.findall(r"^\s*global_(?:load|store|atomic)", m.group(2), re.M)) >= 5, name


# ---- drop-in level and CLI: snappy_decompress_range_gpu and dpu_snappy -d -r against host-mode -r ----

def _cli_range(args, tmp_path, tag):
    from test_cli import CLI, HOST_DIR
    subprocess.check_call(["make", "-s", "-C", HOST_DIR])
    out = tmp_path / tag
    r = subprocess.run([CLI, *args, "-o", str(out)], capture_output=True, text=True)
    return r, (out.read_bytes() if out.exists() else None)


def test_gpu_dropin_and_cli_range_match_host_mode(shb, tmp_path):
    import standins
    spam = tmp_path / "spamfile_like.snappy"
    plain = standins.spamfile_like(standins.prose_texts())
    assert len(plain) == standins.SPAMFILE_LIKE_BYTES
    st, stream, _ = shb.compress_host(plain, 32768)
    assert st == 0
    spam.write_bytes(stream)
    rng = np.random.default_rng(84)
    for path in (os.path.join(ROOT, "tests", "golden", "xml.snappy"), str(spam)):
        data = open(path, "rb").read()
        total = shb.parse_header(data[:10])[0]
        cases = [(0, 1), (32767, 2), (total - 1, 1), (0, total), (12345, 0)]
        cases += [(int(o), int(min(total - o, n))) for o, n in zip(rng.integers(0, total, 4), rng.integers(1, 1 << 21, 4))]
        for k, (off, n) in enumerate(cases):
            st, got, rt = shb.decompress_range_host(data, off, n)
            assert st == 0, (path, off, n)
            assert set(rt) >= {"pre", "d_alloc", "load", "copy_in", "run", "copy_out", "d_free"}
            r_h, host = _cli_range(["-r", f"{off}:{n}", "-i", path], tmp_path, f"h{k}")
            r_d, dev = _cli_range(["-d", "-r", f"{off}:{n}", "-i", path], tmp_path, f"d{k}")
            assert r_h.returncode == 0 and r_d.returncode == 0, (r_h.stderr, r_d.stderr)
            assert len(got) == n and got == host == dev, (path, off, n)
    # a caller-owned output buffer too small for the range; a range beyond the container
    data = open(os.path.join(ROOT, "tests", "golden", "xml.snappy"), "rb").read()
    st, _, _ = shb.decompress_range_host(data, 10, 100, out_capacity=99)
    assert st == shb.SNAPPY_BUFFER_TOO_SMALL
    st, got, _ = shb.decompress_range_host(data, 10, 100, out_capacity=100)
    assert st == 0 and len(got) == 100
    st, _, _ = shb.decompress_range_host(data, 5345280, 1)
    assert st == shb.SNAPPY_INVALID_INPUT
    r_d, dev = _cli_range(["-d", "-r", "5345280:1", "-i", os.path.join(ROOT, "tests", "golden", "xml.snappy")], tmp_path, "beyond")
    assert r_d.returncode != 0 and r_d.stderr.strip() and dev is None
    # coding.txt at 1000-byte blocks, a span through blocks 2..4: each damaged variant gets the status that the front end's CPU
    # test (tests/test_dropin_plan.py) holds to the model -- decided on the host, so damage behind block 4 does not matter
    plain = golden_bytes("coding.txt")
    stream = oracle.compress(plain, 1000)
    off, n = cc.inner_span(1000)
    variants = cc.damaged(stream)
    variants["cut after block 4"] = stream[:cc.chain(stream)[5]]
    for kind, bad in variants.items():
        st, got, _ = shb.decompress_range_host(bad, off, n)
        assert st == cc.model(bad, off, n, update=False)[0], kind
        assert got == (plain[off:off + n] if st == 0 else b""), kind
    served = [kind for kind, bad in variants.items() if cc.model(bad, off, n, update=False)[0] == 0]
    assert served == ["intact", "cut in a size prefix", "cut in a body", "7 trailing bytes", "a middle size field of 0x7ffffff0",
                      "cut after block 4"]
    st, _, _ = shb.decompress_range_host(stream, off, n, out_capacity=n - 1)
    assert st == shb.SNAPPY_BUFFER_TOO_SMALL
    st, got, _ = shb.decompress_range_host(stream, off, n, out_capacity=n)
    assert st == 0 and got == plain[off:off + n]
