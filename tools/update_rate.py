#!/usr/bin/env python3
"""Rate of snappy_hip_update_ranges on one resident 1 GiB Silesia-mix container at 32 KiB blocks.
The container is compressed and indexed once; then batches of seeded, sorted, disjoint writes of random bytes (4 KiB: 1k, 8k,
16k and 64k of them, where 16k brackets the crossover with the full path; 1 MiB: 1k) are applied, each batch timed with HIP
events around the call (one warm-up call, best of three), and every batch's new stream is verified by a full decode against
the plaintext with the writes applied.  Beside it the time of the full path for the same container -- decode all, overlay,
compress all, compact -- which uses only calls that exist without the update (--full-only runs nothing else, so the same
script times it from an older build of the library).
One JSON line per batch: dirty blocks, ms of the call, dirty blocks/s, ms of the full path.
--prof: one call per batch and one full path, nothing else -- the run to put under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/update_rate.py [--prof] [--full-only] [--out FILE]
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
    ap.add_argument("--full-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    with open(os.path.join(silesia_mix.GOLDEN, "xml.snappy"), "rb") as f:
        st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(f.read(), dtype=np.uint8).copy()).cuda())
    assert st == 0 and hashlib.sha256(d_xml.cpu().numpy().tobytes()).hexdigest() == silesia_mix.XML_TXT_SHA256
    unit = torch.from_numpy(silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0).copy()).cuda()
    d_plain = silesia_mix.container_from_unit(unit, GIB)
    d_stream = shb.compress_resident(d_plain, BS, n=GIB)
    total, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
    nb = shb.num_blocks(total, bs)
    d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_desc = shb.make_stream_descs([dict(stream=d_stream, stream_len=d_stream.numel(), block_offsets=d_boff, result=d_res, total_len=total,
                                         block_size=bs, header_len=hdr, num_blocks=nb)])
    shb.index_streams(d_desc, 1)
    torch.cuda.synchronize()
    assert int(d_res[0].item()) == 0
    reps = 1 if args.prof else 3

    # the full path: decode all, overlay one write, compress all, compact (its time does not depend on the writes)
    ws = shb.CompressWorkspace(GIB, BS)
    d_out = torch.empty(GIB + 16, dtype=torch.uint8, device="cuda")
    d_status = torch.empty(nb, dtype=torch.int32, device="cuda")
    d_full_stream = torch.empty(ws.stream_capacity(GIB) + 16, dtype=torch.uint8, device="cuda")
    d_one = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def full_path():
        shb.decompress_blocks(d_stream, d_stream.numel(), d_boff, total, bs, d_out, d_status)
        d_out[12345:12345 + 4096].copy_(d_one)
        shb.compress_blocks(d_out, GIB, ws)
        shb.compact(GIB, ws, d_full_stream)

    if not args.prof:
        full_path()
    full_ms = round(timed(full_path, reps) * 1e3, 3)
    assert int((d_status != 0).sum().item()) == 0
    print(json.dumps({"full_path_ms": full_ms, "blocks": nb}), flush=True)
    rows = [{"full_path_ms": full_ms, "blocks": nb}]
    del d_out, d_full_stream, ws
    if args.full_only:
        return 0

    d_new = torch.empty(10 + nb * shb.slot_stride(BS), dtype=torch.uint8, device="cuda")        # every block at its worst case
    d_noff = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_result = torch.zeros(2, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(20261016)
    for size, count in ((4 << 10, 1000), (4 << 10, 8000), (4 << 10, 16000), (4 << 10, 64000), (1 << 20, 1000)):
        if args.prof and count in (16000, 64000):
            continue
        # sorted and disjoint: distinct cells of a grid of `size` bytes, all shifted by the same odd amount (a 4 KiB write
        # straddles a block boundary in one case of eight)
        shift = int(rng.integers(1, size)) | 1
        cells = np.sort(rng.choice(total // size - 1, count, replace=False)).astype(np.int64)
        offs = cells * size + shift
        d_src = torch.from_numpy(rng.integers(0, 256, count * size, dtype=np.uint8)).cuda()
        d_writes = shb.make_writes([(int(o), size, d_src.data_ptr() + i * size) for i, o in enumerate(offs)])
        d_wstatus = torch.empty(count, dtype=torch.int32, device="cuda")
        dirty = int(np.unique(np.concatenate([np.arange(o // BS, (o + size - 1) // BS + 1) for o in offs])).size)
        scratch = torch.empty(shb.update_scratch_bytes(BS, nb, count, dirty), dtype=torch.uint8, device="cuda")

        def call():
            shb.update_ranges(d_desc, total, BS, d_writes, count, d_wstatus, d_new, d_noff, d_len, d_result, dirty, d_scratch=scratch)

        if not args.prof:
            call()
        best = timed(call, reps)
        assert [int(x) for x in d_result.cpu().numpy()] == [0, dirty] and int((d_wstatus != 0).sum().item()) == 0
        # verified by a full decode against the plaintext with the writes applied
        st, d_back = shb.decompress_resident(d_new[:int(d_len.item())])
        assert st == 0
        d_want = d_plain[:GIB].clone()
        view = d_src.view(count, size)
        step = max(1, (64 << 20) // size)
        ar = torch.arange(size, device="cuda")
        d_offs = torch.from_numpy(offs).cuda()
        for lo in range(0, count, step):
            d_want[d_offs[lo:lo + step, None] + ar[None, :]] = view[lo:lo + step]
        assert torch.equal(d_back[:GIB], d_want), (size, count)
        row = {"write_bytes": size, "writes": count, "dirty_blocks": dirty, "dirty_share": round(dirty / nb, 4), "ms": round(best * 1e3, 3),
               "dirty_blocks_per_s": round(dirty / best), "full_path_ms": full_ms, "new_stream_bytes": int(d_len.item())}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_src, d_writes, scratch, d_back, d_want
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
