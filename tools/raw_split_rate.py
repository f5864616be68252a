#!/usr/bin/env python3
"""Rate of snappy_hip_raw_decompress_split_batch on ONE large raw stream.  A resident Silesia-mix is
raw-compressed at 32 KiB fragments (snappy_hip_raw_compress_batch, one item) in sizes of 64 MiB, 256 MiB and 1 GiB; the one
stream is decoded by the split call at unit_len 65,536 with segments of 16, 64 and 256 KiB.  Each call is timed with HIP
events around it: one warm-up call, then three, of which the best and the spread (slowest - fastest) are reported; every run
is verified: status OK, d_result = [1, 0, 0, 0], the decoded bytes equal the source.  Beside it, on the same bytes: the
serial call (snappy_hip_raw_decompress_batch, one wavefront) for the 64 MiB item only, and snappy_hip_decompress_blocks of
the framed form at 32 KiB blocks as the ceiling.  One JSON line per measurement.
--prof: one split call on the 64 MiB item per segment size and nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats` for the per-step times.
Usage: python tools/raw_split_rate.py [--prof] [--sizes-mib 64,256,1024] [--out FILE]
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

MIB, BS, UNIT = 1 << 20, 32768, 65536
SEGMENTS = (16 << 10, 64 << 10, 256 << 10)


def timed(call, reps, before=None, after=None):
    """-> sorted seconds of `reps` calls"""
    import torch
    out = []
    for _ in range(reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / 1e3)
        if after:
            after()
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--sizes-mib", default="64,256,1024")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    sizes = [int(x) * MIB for x in args.sizes_mib.split(",")]
    if args.prof:
        sizes = sizes[:1]
    with open(os.path.join(silesia_mix.GOLDEN, "xml.snappy"), "rb") as f:
        st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(f.read(), dtype=np.uint8).copy()).cuda())
    assert st == 0 and hashlib.sha256(d_xml.cpu().numpy().tobytes()).hexdigest() == silesia_mix.XML_TXT_SHA256
    unit = torch.from_numpy(silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0).copy()).cuda()
    d_in = silesia_mix.container_from_unit(unit, max(sizes))
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def ms(ts):
        return {"ms": round(ts[0] * 1e3, 3), "spread_ms": round((ts[-1] - ts[0]) * 1e3, 3)}

    for size in sizes:
        label = "1 x %d MiB" % (size // MIB)
        # ---- the one raw stream ----
        bound = shb.raw_compress_bound(size, BS)
        frags = (size + BS - 1) // BS
        comp = torch.empty(bound, dtype=torch.uint8, device="cuda")
        plain = torch.empty(size + 16, dtype=torch.uint8, device="cuda")[:size]
        d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_status = torch.empty(1, dtype=torch.int32, device="cuda")
        d_result = torch.zeros(4, dtype=torch.int32, device="cuda")
        shb.raw_compress_batch(shb.make_raw_items([(d_in.data_ptr(), size, comp.data_ptr(), bound)]), 1, BS, frags, d_len, d_status, d_result[:2])
        assert int(d_status.item()) == 0
        clen = int(d_len.item())
        items = shb.make_raw_items([(comp.data_ptr(), clen, plain.data_ptr(), size)])
        d_len2 = torch.zeros(1, dtype=torch.int64, device="cuda")

        def verify(want_result=None):
            assert int(d_status.item()) == 0 and int(d_len2.item()) == size, (label, int(d_status.item()))
            if want_result:
                assert d_result.cpu().tolist() == want_result, (label, d_result.cpu().tolist())
            assert torch.equal(plain, d_in[:size]), label

        def reset():
            plain.fill_(0xA5)
            d_status.fill_(0x55)

        split_ms = {}
        for seg in SEGMENTS:
            max_segments, max_units = clen // seg + 1, size // UNIT + 1
            scratch = torch.empty(shb.raw_decompress_split_scratch_bytes(1, UNIT, seg, max_segments, max_units), dtype=torch.uint8, device="cuda")

            def do_split():
                shb.raw_decompress_split_batch(items, 1, UNIT, seg, max_segments, max_units, d_len2, d_status, d_result, scratch)
            if not args.prof:
                reset()
                do_split()
                verify([1, 0, 0, 0])
            ts = timed(do_split, 1 if args.prof else 3, before=reset, after=lambda: verify([1, 0, 0, 0]))
            split_ms[seg] = ts
            emit({"what": "split decode, " + label, "segment_bytes": seg, "unit_len": UNIT, "compressed_bytes": clen, "scratch_bytes": scratch.numel(),
                  **ms(ts), "GBps": round(size / ts[0] / 1e9, 3)})
            del scratch
        if args.prof:
            continue
        best_seg = min(split_ms, key=lambda s: split_ms[s][0])
        # ---- the serial call on the same stream (one wavefront; about a second per 64 MiB: the smallest item only) ----
        t_serial = None
        if size == sizes[0]:
            def do_serial():
                shb.raw_decompress_batch(items, 1, d_len2, d_status)
            reset()
            do_serial()
            verify()
            t_serial = timed(do_serial, 3, before=reset, after=verify)
            emit({"what": "serial decode (raw_decompress_batch), " + label, **ms(t_serial), "GBps": round(size / t_serial[0] / 1e9, 4)})
        # ---- the ceiling: the framed form of the same bytes ----
        ws = shb.CompressWorkspace(size, BS)
        d_stream = torch.empty(ws.stream_capacity(size) + 16, dtype=torch.uint8, device="cuda")
        shb.compress_blocks(d_in, size, ws)
        shb.compact(size, ws, d_stream)
        stream_len = int(ws.stream_len.item())
        total, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
        nb = shb.num_blocks(total, bs)
        d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
        d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
        descs = shb.make_stream_descs([dict(stream=d_stream, stream_len=stream_len, block_offsets=d_boff, result=d_res, total_len=total,
                                            block_size=bs, header_len=hdr, num_blocks=nb)])
        shb.index_streams(descs, 1)
        d_bst = torch.empty(nb, dtype=torch.int32, device="cuda")

        def framed_decode():
            shb.decompress_blocks(d_stream, stream_len, d_boff, total, bs, plain, d_bst)
        framed_decode()
        t_k2 = timed(framed_decode, 3, before=lambda: plain.fill_(0xA5))
        assert int((d_bst != 0).sum().item()) == 0 and torch.equal(plain, d_in[:size])
        emit({"what": "ceiling decompress_blocks of the framed form, " + label, **ms(t_k2), "GBps": round(size / t_k2[0] / 1e9, 2)})
        row = {"what": "summary, " + label, "best_segment_bytes": best_seg, "split_ms": round(split_ms[best_seg][0] * 1e3, 3),
               "ceiling_over_split": round(split_ms[best_seg][0] / t_k2[0], 2)}
        if t_serial:
            row["serial_over_split"] = round(t_serial[0] / split_ms[best_seg][0], 1)
            # faster by more than the spread of the three runs of either
            row["faster_beyond_spread"] = bool(t_serial[0] - split_ms[best_seg][-1] > max(t_serial[-1] - t_serial[0], split_ms[best_seg][-1] - split_ms[best_seg][0]))
        emit(row)
        del ws, d_stream, d_boff, d_bst, comp, plain
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
