#!/usr/bin/env python3
"""Rate of snappy_hip_decompress_ranges on the resident 8 x 1 GiB Silesia-mix.
The eight containers are compressed once and indexed once; then batches of seeded random ranges (4 KiB, 64 KiB, 1 MiB;
1k, 8k and 64k of them, spread over the eight containers) are decoded, each batch timed with HIP events around the call
(one warm-up call, best of three), and every batch's output is checked against a full decode of the same streams.
One JSON line per batch: ranges/s, delivered GB/s (bytes asked for), decoded-block GB/s (bytes of the blocks touched).
--prof: one call per batch and one full K2 decode of the eight containers, nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats` for the per-block kernel times of decompress_ranges_kernel and decompress_blocks_kernel.
Usage: python tools/range_rate.py [--prof] [--out FILE]
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

CONTAINERS, GIB, BS = 8, 1 << 30, 32768


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
    # the eight containers: the unit rotated by a different amount each, so that no two hold the same blocks
    ref = torch.empty(CONTAINERS * GIB, dtype=torch.uint8, device="cuda")   # full decodes, end to end
    streams, entries = [], []
    for k in range(CONTAINERS):
        d_in = silesia_mix.container_from_unit(torch.roll(unit, k * 1234567), GIB)
        d_stream = shb.compress_resident(d_in, BS, n=GIB)
        st, d_full = shb.decompress_resident(d_stream)
        assert st == 0 and torch.equal(d_full[:GIB], d_in[:GIB])
        ref[k * GIB:(k + 1) * GIB] = d_full[:GIB]
        del d_in, d_full
        total, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
        nb = shb.num_blocks(total, bs)
        d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
        streams.append((d_stream, d_boff))
        entries.append(dict(stream=d_stream, stream_len=d_stream.numel(), block_offsets=d_boff,
                            result=torch.zeros(2, dtype=torch.int32, device="cuda"), total_len=total, block_size=bs, header_len=hdr,
                            num_blocks=nb))
    descs = shb.make_stream_descs(entries)
    shb.index_streams(descs, CONTAINERS)
    torch.cuda.synchronize()
    assert all(int(e["result"][0].item()) == 0 for e in entries)
    scratch = torch.empty(shb.decompress_ranges_scratch_bytes(BS, 1 << 16), dtype=torch.uint8, device="cuda")

    rows = []
    rng = np.random.default_rng(20261016)
    for size in (4 << 10, 64 << 10, 1 << 20):
        for count in (1000, 8000, 64000):
            if args.prof and count != 8000:
                continue
            cont = rng.integers(0, CONTAINERS, count)
            offs = rng.integers(0, GIB - size + 1, count)
            buf = torch.empty(count * size, dtype=torch.uint8, device="cuda")
            d_ranges = shb.make_ranges([(int(c), int(o), size, buf.data_ptr() + i * size) for i, (c, o) in enumerate(zip(cont, offs))])
            d_status = torch.empty(count, dtype=torch.int32, device="cuda")
            first, last = offs // BS, (offs + size - 1) // BS
            pieces = int((last - first + 1).sum())
            block_bytes = int((np.minimum(GIB, (last + 1) * BS) - first * BS).sum())
            reps = 1 if args.prof else 3
            if not args.prof:
                shb.decompress_ranges(descs, CONTAINERS, d_ranges, count, d_status, BS, scratch)     # warm-up
            best = 1e9
            for _ in range(reps):
                buf.fill_(0xA5)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                shb.decompress_ranges(descs, CONTAINERS, d_ranges, count, d_status, BS, scratch)
                e1.record()
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1) / 1e3)
            assert int((d_status != 0).sum().item()) == 0
            # check against the full decodes: gather each range's bytes from `ref`, a few MiB of indices at a time
            src = torch.from_numpy(cont.astype(np.int64) * GIB + offs.astype(np.int64)).cuda()
            view = buf.view(count, size)
            step = max(1, (64 << 20) // size)
            ar = torch.arange(size, device="cuda")
            for lo in range(0, count, step):
                idx = src[lo:lo + step, None] + ar[None, :]
                assert torch.equal(view[lo:lo + step], ref[idx]), (size, count, lo)
            row = {"range_bytes": size, "ranges": count, "pieces": pieces, "ms": round(best * 1e3, 3),
                   "ranges_per_s": round(count / best), "delivered_GBps": round(count * size / best / 1e9, 2),
                   "decoded_block_GBps": round(block_bytes / best / 1e9, 2), "blocks_per_range": round(pieces / count, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del buf, d_ranges, d_status
    if args.prof:
        # one full K2 decode of the eight containers, for the kernel statistics beside the range kernel's
        jobs = []
        for k, (d_stream, d_boff) in enumerate(streams):
            nb = entries[k]["num_blocks"]
            jobs.append((d_stream, d_stream.numel(), d_boff, GIB, ref[k * GIB:(k + 1) * GIB],
                         torch.empty(nb, dtype=torch.int32, device="cuda")))
        shb.decompress_blocks_batch(jobs, BS)
        torch.cuda.synchronize()
        assert all(int((j[5] != 0).sum().item()) == 0 for j in jobs)
        print(json.dumps({"k2_blocks": sum(e["num_blocks"] for e in entries)}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
