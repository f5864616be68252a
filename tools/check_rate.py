#!/usr/bin/env python3
"""What does a check cost beside a decode?  Two cases on a resident 1 GiB Silesia-mix:
  * the container at 32 KiB blocks: snappy_hip_check_blocks beside snappy_hip_decompress_blocks on the same stream and
    offsets, in the same run, alternating (check, decode, check, decode, ...); the figure is the ratio of the two times;
  * 8192 raw items of 64 KiB, carved from the mix at seeded offsets and compressed at 32 KiB fragments:
    snappy_hip_raw_check_batch beside snappy_hip_raw_decompress_batch, alternating.
Each call is timed with HIP events around it (one warm-up call each, best of three) and every result is verified: the
decode's statuses all OK and its bytes equal to the source, the check's result words [OK, 0, 0xffffffff, 0] and its
per-block statuses equal to the decode's; the raw check's (status, length) equal to the raw decode's.  Then the same
container with 1000 seeded damaged bytes: the check's per-block statuses against the decode's again (not timed).
One JSON line per measurement.
Usage: python tools/check_rate.py [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pim-compression_amd"))
import silesia_mix  # noqa: E402
import snappy_hip_binding as shb  # noqa: E402

GIB, BS = 1 << 30, 32768


def timed_once(call):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3


def alternating(a, b, reps=3):
    """one warm-up call each, then a, b, a, b, ...: best of `reps` for each"""
    a()
    b()
    ta = tb = 1e9
    for _ in range(reps):
        ta = min(ta, timed_once(a))
        tb = min(tb, timed_once(b))
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    with open(os.path.join(silesia_mix.GOLDEN, "xml.snappy"), "rb") as f:
        st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(f.read(), dtype=np.uint8).copy()).cuda())
    assert st == 0 and hashlib.sha256(d_xml.cpu().numpy().tobytes()).hexdigest() == silesia_mix.XML_TXT_SHA256
    unit = torch.from_numpy(silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0).copy()).cuda()
    d_in = silesia_mix.container_from_unit(unit, GIB)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- the framed container ----
    ws = shb.CompressWorkspace(GIB, BS)
    d_stream = torch.empty(ws.stream_capacity(GIB) + 16, dtype=torch.uint8, device="cuda")
    shb.compress_blocks(d_in, GIB, ws)
    shb.compact(GIB, ws, d_stream)
    stream_len = int(ws.stream_len.item())
    del ws
    total, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
    nb = shb.num_blocks(total, bs)
    d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    descs = shb.make_stream_descs([dict(stream=d_stream, stream_len=stream_len, block_offsets=d_boff, result=d_res, total_len=total,
                                        block_size=bs, header_len=hdr, num_blocks=nb)])
    shb.index_streams(descs, 1)
    assert [int(x) for x in d_res.cpu().numpy()] == [0, nb]
    d_full = torch.empty(GIB + 16, dtype=torch.uint8, device="cuda")
    d_k2 = torch.empty(nb, dtype=torch.int32, device="cuda")
    d_chk = torch.empty(nb, dtype=torch.int32, device="cuda")
    d_ptr = torch.from_numpy(np.array([d_chk.data_ptr()], dtype=np.int64)).cuda()
    d_results = torch.empty(4, dtype=torch.int32, device="cuda")
    scratch = torch.empty(shb.check_scratch_bytes(1), dtype=torch.uint8, device="cuda")

    def decode():
        shb.decompress_blocks(d_stream, stream_len, d_boff, total, bs, d_full, d_k2)

    def check():
        shb.check_blocks(descs, 1, d_results, d_ptr, scratch)

    def check_bare():
        shb.check_blocks(descs, 1, d_results, None, scratch)

    t_chk, t_k2 = alternating(check, decode)
    assert int((d_k2 != 0).sum().item()) == 0 and torch.equal(d_full[:GIB], d_in[:GIB])
    assert [int(x) & 0xffffffff for x in d_results.cpu().numpy()] == [0, 0, 0xffffffff, 0] and torch.equal(d_chk, d_k2)
    emit({"what": "1 GiB Silesia-mix container, 32 KiB blocks: check_blocks (with per-block statuses) beside decompress_blocks, alternating",
          "blocks": nb, "stream_bytes": stream_len, "check_ms": round(t_chk * 1e3, 3), "decode_ms": round(t_k2 * 1e3, 3),
          "check_GBps_of_plaintext": round(GIB / t_chk / 1e9, 2), "check_GBps_of_stream": round(stream_len / t_chk / 1e9, 2),
          "decode_GBps_of_plaintext": round(GIB / t_k2 / 1e9, 2), "check_over_decode": round(t_chk / t_k2, 4)})
    t_bare, t_k2b = alternating(check_bare, decode)
    assert [int(x) & 0xffffffff for x in d_results.cpu().numpy()] == [0, 0, 0xffffffff, 0]
    emit({"what": "the same without a status array", "check_ms": round(t_bare * 1e3, 3), "decode_ms": round(t_k2b * 1e3, 3),
          "check_over_decode": round(t_bare / t_k2b, 4)})
    # the same container with 1000 damaged bytes: block for block against the decode
    rng = np.random.default_rng(1000)
    at = torch.from_numpy(rng.integers(hdr, stream_len, 1000).astype(np.int64)).cuda()
    d_stream[at] ^= torch.from_numpy(rng.integers(1, 256, 1000).astype(np.uint8)).cuda()
    decode()
    check()
    torch.cuda.synchronize()
    bad = int((d_k2 != 0).sum().item())
    first = int(torch.nonzero(d_k2 != 0)[0].item())
    assert torch.equal(d_chk, d_k2) and [int(x) & 0xffffffff for x in d_results.cpu().numpy()] == [1, bad, first, 0] and bad > 100
    emit({"what": "the same container with 1000 seeded damaged bytes (not timed): per-block statuses equal to the decode's", "invalid_blocks": bad,
          "first_invalid_block": first})
    del d_stream, d_full, d_boff, d_k2, d_chk

    # ---- raw items ----
    size, count = 64 << 10, 8192
    bound = shb.raw_compress_bound(size, BS)
    frags = count * ((size + BS - 1) // BS)
    offs = np.random.default_rng(size + count).integers(0, GIB - size + 1, count).astype(np.int64)
    comp = torch.empty(count * bound, dtype=torch.uint8, device="cuda")
    plain = torch.empty(count * size, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(count, dtype=torch.int64, device="cuda")
    d_status = torch.empty(count, dtype=torch.int32, device="cuda")
    d_result = torch.zeros(2, dtype=torch.int32, device="cuda")
    items_c = shb.make_raw_items([(d_in.data_ptr() + int(o), size, comp.data_ptr() + i * bound, bound) for i, o in enumerate(offs)])
    shb.raw_compress_batch(items_c, count, BS, frags, d_len, d_status, d_result)
    assert [int(x) for x in d_result.cpu().numpy()] == [frags, count] and int((d_status != 0).sum().item()) == 0
    lens = d_len.cpu().numpy()
    items_d = shb.make_raw_items([(comp.data_ptr() + i * bound, int(lens[i]), plain.data_ptr() + i * size, size) for i in range(count)])
    items_k = shb.make_raw_items([(comp.data_ptr() + i * bound, int(lens[i]), 0, 0) for i in range(count)])
    d_len_d, d_len_k = torch.zeros(count, dtype=torch.int64, device="cuda"), torch.zeros(count, dtype=torch.int64, device="cuda")
    d_st_d, d_st_k = torch.empty(count, dtype=torch.int32, device="cuda"), torch.empty(count, dtype=torch.int32, device="cuda")

    def raw_decode():
        shb.raw_decompress_batch(items_d, count, d_len_d, d_st_d)

    def raw_check():
        shb.raw_check_batch(items_k, count, d_len_k, d_st_k)

    t_rc, t_rd = alternating(raw_check, raw_decode)
    assert int((d_st_d != 0).sum().item()) == 0 and int((d_len_d != size).sum().item()) == 0
    assert torch.equal(d_st_k, d_st_d) and torch.equal(d_len_k, d_len_d)
    src = torch.from_numpy(offs).cuda()
    view, ar = plain.view(count, size), torch.arange(size, device="cuda")
    for lo in range(0, count, 1024):
        assert torch.equal(view[lo:lo + 1024], d_in[src[lo:lo + 1024, None] + ar[None, :]]), lo
    emit({"what": "8192 raw items of 64 KiB: raw_check_batch beside raw_decompress_batch, alternating", "compressed_bytes": int(lens.sum()),
          "check_ms": round(t_rc * 1e3, 3), "decode_ms": round(t_rd * 1e3, 3), "check_GBps_of_plaintext": round(count * size / t_rc / 1e9, 2),
          "decode_GBps_of_plaintext": round(count * size / t_rd / 1e9, 2), "check_over_decode": round(t_rc / t_rd, 4)})
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
