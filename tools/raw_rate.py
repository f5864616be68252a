#!/usr/bin/env python3
"""Rates of snappy_hip_raw_compress_batch / snappy_hip_raw_decompress_batch on a resident 1 GiB Silesia-mix.
Batches of 1k / 8k / 64k items of 64 KiB and of 1 MiB, carved from the mix at seeded offsets (items may share source bytes;
every item has an output of its own), compressed at 32 KiB fragments and decoded again; then ONE item of 1 GiB.  Each call is
timed with HIP events around it (one warm-up call, best of three; the single stream once) and every batch is verified: all
items OK, and the decoded bytes equal the source.  A batch whose buffers would not fit the device's free memory is reported as skipped, not shrunk.
In the same run, the yardsticks from the entry points that existed before, on the same 1 GiB: snappy_hip_decompress_blocks
of the framed form at 32 KiB blocks, and snappy_hip_compress_blocks with SNAPPY_HIP_COMPRESS_VARIANT=1 (the LDS-table kernel
alone, the form the fragments are compressed with) + snappy_hip_compact.  One JSON line per measurement.
--prof: one call of each kind on the 8k x 64 KiB batch and one full K2 decode, nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats`.
Usage: python tools/raw_rate.py [--prof] [--out FILE]
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


def timed(call, reps, before=None):
    import torch
    best = 1e9
    for _ in range(reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    with open(os.path.join(silesia_mix.GOLDEN, "xml.snappy"), "rb") as f:
        st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(f.read(), dtype=np.uint8).copy()).cuda())
    assert st == 0 and hashlib.sha256(d_xml.cpu().numpy().tobytes()).hexdigest() == silesia_mix.XML_TXT_SHA256
    unit = torch.from_numpy(silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0).copy()).cuda()
    d_in = silesia_mix.container_from_unit(unit, GIB)
    rows = []
    reps = 1 if args.prof else 3

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- yardsticks: the framed form of the same 1 GiB ----
    os.environ["SNAPPY_HIP_COMPRESS_VARIANT"] = "1"
    ws = shb.CompressWorkspace(GIB, BS)
    d_stream = torch.empty(ws.stream_capacity(GIB) + 16, dtype=torch.uint8, device="cuda")

    def framed_compress():
        shb.compress_blocks(d_in, GIB, ws)
        shb.compact(GIB, ws, d_stream)
    if not args.prof:
        framed_compress()
    t_k1 = timed(framed_compress, reps)
    del os.environ["SNAPPY_HIP_COMPRESS_VARIANT"]
    stream_len = int(ws.stream_len.item())
    total, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
    nb = shb.num_blocks(total, bs)
    d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    descs = shb.make_stream_descs([dict(stream=d_stream, stream_len=stream_len, block_offsets=d_boff, result=d_res, total_len=total,
                                        block_size=bs, header_len=hdr, num_blocks=nb)])
    shb.index_streams(descs, 1)
    d_full = torch.empty(GIB + 16, dtype=torch.uint8, device="cuda")
    d_bst = torch.empty(nb, dtype=torch.int32, device="cuda")

    def framed_decode():
        shb.decompress_blocks(d_stream, stream_len, d_boff, total, bs, d_full, d_bst)
    if not args.prof:
        framed_decode()
    t_k2 = timed(framed_decode, reps)
    assert int((d_bst != 0).sum().item()) == 0 and torch.equal(d_full[:GIB], d_in[:GIB])
    k1_gbps, k2_gbps = GIB / t_k1 / 1e9, GIB / t_k2 / 1e9
    emit({"what": "yardstick compress_blocks(variant 1) + compact, 1 GiB, 32 KiB blocks", "ms": round(t_k1 * 1e3, 3), "GBps": round(k1_gbps, 2)})
    emit({"what": "yardstick decompress_blocks, 1 GiB, 32 KiB blocks", "ms": round(t_k2 * 1e3, 3), "GBps": round(k2_gbps, 2)})
    del ws, d_stream, d_full, d_boff, d_bst

    def batch(size, count, label):
        bound = shb.raw_compress_bound(size, BS)
        frags = count * ((size + BS - 1) // BS)
        need = count * (bound + size) + shb.raw_compress_scratch_bytes(BS, count, frags)
        free = torch.cuda.mem_get_info()[0]
        if need > free * 0.9:
            emit({"what": label, "skipped": "needs %.1f GiB of device memory, %.1f GiB free" % (need / GIB, free / GIB)})
            return
        rng = np.random.default_rng(size + count)
        offs = rng.integers(0, GIB - size + 1, count).astype(np.int64)
        comp = torch.empty(count * bound, dtype=torch.uint8, device="cuda")
        plain = torch.empty(count * size, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(shb.raw_compress_scratch_bytes(BS, count, frags), dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(count, dtype=torch.int64, device="cuda")
        d_status = torch.empty(count, dtype=torch.int32, device="cuda")
        d_result = torch.zeros(2, dtype=torch.int32, device="cuda")
        items_c = shb.make_raw_items([(d_in.data_ptr() + int(o), size, comp.data_ptr() + i * bound, bound) for i, o in enumerate(offs)])

        def do_compress():
            shb.raw_compress_batch(items_c, count, BS, frags, d_len, d_status, d_result, scratch)
        one = count == 1                                     # (the single stream takes seconds: one timed call, no warm-up)
        if not args.prof and not one:
            do_compress()
        t_c = timed(do_compress, 1 if one else reps)
        assert [int(x) for x in d_result.cpu().numpy()] == [frags, count] and int((d_status != 0).sum().item()) == 0
        lens = d_len.cpu().numpy()
        items_d = shb.make_raw_items([(comp.data_ptr() + i * bound, int(lens[i]), plain.data_ptr() + i * size, size) for i in range(count)])
        d_len2 = torch.zeros(count, dtype=torch.int64, device="cuda")

        def do_decode():
            shb.raw_decompress_batch(items_d, count, d_len2, d_status)
        if not args.prof and not one:
            do_decode()
        t_d = timed(do_decode, 1 if one else reps, before=lambda: plain.fill_(0xA5))
        assert int((d_status != 0).sum().item()) == 0 and int((d_len2 != size).sum().item()) == 0
        # verified against the source: gather each item's bytes from the mix, a few MiB of indices at a time
        src = torch.from_numpy(offs).cuda()
        view = plain.view(count, size)
        step = max(1, (64 << 20) // size)
        ar = None if one else torch.arange(size, device="cuda")
        for lo in range(0, 0 if one else count, step):
            assert torch.equal(view[lo:lo + step], d_in[src[lo:lo + step, None] + ar[None, :]]), (label, lo)
        if one:
            assert torch.equal(plain, d_in[int(offs[0]):int(offs[0]) + size]), label
        nbytes = count * size
        emit({"what": label, "item_bytes": size, "items": count, "compressed_bytes": int(lens.sum()),
              "compress_ms": round(t_c * 1e3, 3), "compress_GBps": round(nbytes / t_c / 1e9, 2), "compress_vs_yardstick": round(nbytes / t_c / 1e9 / k1_gbps, 3),
              "decode_ms": round(t_d * 1e3, 3), "decode_GBps": round(nbytes / t_d / 1e9, 3), "decode_vs_yardstick": round(nbytes / t_d / 1e9 / k2_gbps, 4)})

    if args.prof:
        batch(64 << 10, 8000, "8000 x 64 KiB")
    else:
        for size in (64 << 10, 1 << 20):
            for count in (1000, 8000, 64000):
                batch(size, count, "%d x %d KiB" % (count, size >> 10))
        batch(GIB, 1, "1 x 1 GiB (one stream: one wavefront decodes it)")
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
