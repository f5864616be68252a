#!/usr/bin/env python3
"""Time of snappy_hip_resize on one resident 1 GiB Silesia-mix container at 32 KiB blocks.
The container is compressed and indexed once.  Then, each timed with HIP events around the call (one warm-up call, best of
three) and each verified by a full decode of the new stream against the new plaintext:
  * an append of 4 KiB, 1 MiB, 64 MiB and 512 MiB of Silesia-mix bytes onto the container cut in the middle of a block
    (keep_len = 1 GiB - 12345), in one segment;
  * a truncate to half (keep_len = 512 MiB + 12345, again in the middle of a block).
Beside each, in the same run, the full path for the same new plaintext with the calls that exist without the resize: decode
all, put the tail behind the kept bytes, compress all (the product's K1 launch), compact.
One JSON line per case: blocks compressed, ms of the call, ms of the full path.
--prof: one call per case and one full path each, nothing else -- the run to put under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/resize_rate.py [--prof] [--out FILE]
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
CUT = 12345


def timed(fn, reps):
    import torch
    best = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
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
    d_plain = silesia_mix.container_from_unit(unit, GIB)
    d_more = silesia_mix.container_from_unit(torch.from_numpy(silesia_mix.build_unit(d_xml.cpu().numpy(), seed=1).copy()).cuda(), GIB // 2)
    d_stream = shb.compress_resident(d_plain, BS, n=GIB)
    total, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
    nb = shb.num_blocks(total, bs)
    assert (total, bs) == (GIB, BS)
    d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_desc = shb.make_stream_descs([dict(stream=d_stream, stream_len=d_stream.numel(), block_offsets=d_boff, result=d_res, total_len=total,
                                         block_size=bs, header_len=hdr, num_blocks=nb)])
    shb.index_streams(d_desc, 1)
    torch.cuda.synchronize()
    assert int(d_res[0].item()) == 0
    reps = 1 if args.prof else 3
    rows = []
    d_status = torch.empty(nb, dtype=torch.int32, device="cuda")
    for name, keep_len, tail_len in (("append", GIB - CUT, 4 << 10), ("append", GIB - CUT, 1 << 20), ("append", GIB - CUT, 64 << 20),
                                     ("append", GIB - CUT, 512 << 20), ("truncate", GIB // 2 + CUT, 0)):
        new_total = keep_len + tail_len
        new_nb = shb.num_blocks(new_total, BS)
        compressed = new_nb - keep_len // BS
        d_tail = d_more[:tail_len] if tail_len else None
        d_segments = shb.make_segments([(d_tail.data_ptr(), tail_len)] if tail_len else [])
        count = 1 if tail_len else 0
        d_sstatus = torch.empty(1, dtype=torch.int32, device="cuda")
        # a kept block keeps its size, a compressed one grows to a slot at most
        d_new = torch.empty(d_stream.numel() + 16 + compressed * shb.slot_stride(BS), dtype=torch.uint8, device="cuda")
        d_noff = torch.empty(new_nb + 1, dtype=torch.int64, device="cuda")
        d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_result = torch.zeros(2, dtype=torch.int32, device="cuda")
        scratch = torch.empty(shb.resize_scratch_bytes(BS, nb, new_total, keep_len, count), dtype=torch.uint8, device="cuda")

        def call():
            shb.resize(d_desc, total, BS, keep_len, new_total, d_segments, count, d_sstatus, d_new, d_noff, d_len, d_result, d_scratch=scratch)

        if not args.prof:
            call()
        best = timed(call, reps)
        assert [int(x) for x in d_result.cpu().numpy()] == [0, compressed] and (count == 0 or int(d_sstatus[0].item()) == 0)
        # verified by a full decode against the new plaintext
        d_want = torch.cat([d_plain[:keep_len], d_tail]) if tail_len else d_plain[:keep_len]
        st, d_back = shb.decompress_resident(d_new[:int(d_len.item())])
        assert st == 0 and torch.equal(d_back[:new_total], d_want), (name, tail_len)
        del d_back, d_want

        # the full path for the same new plaintext: decode all, the tail behind the kept bytes, compress all, compact
        ws = shb.CompressWorkspace(new_total, BS)
        d_out = torch.empty(max(GIB, new_total) + 16, dtype=torch.uint8, device="cuda")
        d_full = torch.empty(ws.stream_capacity(new_total) + 16, dtype=torch.uint8, device="cuda")

        def full_path():
            shb.decompress_blocks(d_stream, d_stream.numel(), d_boff, total, BS, d_out, d_status)
            if tail_len:
                d_out[keep_len:new_total].copy_(d_tail)
            shb.compress_blocks(d_out, new_total, ws)
            shb.compact(new_total, ws, d_full)

        if not args.prof:
            full_path()
        full = timed(full_path, reps)
        assert int((d_status != 0).sum().item()) == 0
        n_full = int(ws.stream_len.item())
        assert n_full == int(d_len.item()) and torch.equal(d_full[:n_full], d_new[:n_full]), (name, tail_len)
        row = {"case": name, "keep_len": keep_len, "tail_bytes": tail_len, "blocks_compressed": compressed, "ms": round(best * 1e3, 3),
               "full_path_ms": round(full * 1e3, 3), "new_stream_bytes": n_full}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del ws, d_out, d_full, d_new, scratch
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
