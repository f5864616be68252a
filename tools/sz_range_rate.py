#!/usr/bin/env python3
"""snappy_hip_sz_index_batch and snappy_hip_sz_decompress_ranges next to their yardsticks in the same run: the
resident 1 GiB Silesia-mix as ONE .sz stream of 32 KiB chunks (3.13's item) and, for the container's rate, the same plaintext as
one 32 KiB-block container.
  (a) the index call against the split call's sizing call (capacities of 0) at segment_bytes of 1 MiB;
  (b) 1k / 8k / 64k seeded ranges of 4 KiB, 64 KiB and 1 MiB, verified and with SNAPPY_HIP_SZ_NO_VERIFY, against
      snappy_hip_decompress_ranges over the container with the same ranges and against snappy_hip_sz_decompress_split_batch of the
      whole stream (what a caller must do without an index).  A cell whose destinations exceed --max-dst-gib is not run and says so.
Every variant is run once and verified (statuses, the bytes of the ranges against the source), then the variants of a cell are
timed in turn, REPS rounds, with HIP events around each call: the minimum, the median and the maximum are reported, each with its
own (max - min) / min run-to-run spread.  One JSON line per cell and variant.
Usage: python tools/sz_range_rate.py [--out FILE] [--only-small] [--max-dst-gib N]
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

GIB, CL, REPS, SEG = 1 << 30, 32768, 7, 1 << 20


def once(call):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    t = sorted(t)
    return {"ms_min": round(t[0], 4), "ms_median": round(t[len(t) // 2], 4), "ms_max": round(t[-1], 4), "spread": round((t[-1] - t[0]) / t[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-small", action="store_true", help="a 64 MiB source and fewer ranges: a rehearsal")
    ap.add_argument("--max-dst-gib", type=float, default=16.0)
    args = ap.parse_args()
    import torch
    total = GIB if not args.only_small else 64 << 20
    with open(os.path.join(silesia_mix.GOLDEN, "xml.snappy"), "rb") as f:
        st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(f.read(), dtype=np.uint8).copy()).cuda())
    assert st == 0 and hashlib.sha256(d_xml.cpu().numpy().tobytes()).hexdigest() == silesia_mix.XML_TXT_SHA256
    unit = torch.from_numpy(silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0).copy()).cuda()
    d_in = silesia_mix.container_from_unit(unit, total)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- the .sz stream ----
    chunks = (total + CL - 1) // CL
    bound = shb.sz_compress_bound(total, CL)
    comp = torch.empty(bound, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_status = torch.empty(1, dtype=torch.int32, device="cuda")
    d_bad = torch.empty(1, dtype=torch.int32, device="cuda")
    d_result = torch.zeros(4, dtype=torch.int32, device="cuda")
    cscratch = torch.empty(shb.sz_compress_scratch_bytes(CL, 1, chunks), dtype=torch.uint8, device="cuda")
    shb.sz_compress_batch(shb.make_raw_items([(d_in.data_ptr(), total, comp.data_ptr(), bound)]), 1, CL, chunks, d_len, d_status, d_result, cscratch)
    assert int(d_status[0]) == 0
    sz_len = int(d_len[0])
    del cscratch
    plain = torch.empty(total, dtype=torch.uint8, device="cuda")
    item_d = shb.make_raw_items([(comp.data_ptr(), sz_len, plain.data_ptr(), total)])
    item_s = shb.make_raw_items([(comp.data_ptr(), sz_len, 0, 0)])
    max_segments = -(-sz_len // SEG)
    split_scratch = torch.empty(shb.sz_decompress_split_scratch_bytes(1, chunks, SEG, max_segments), dtype=torch.uint8, device="cuda")
    d_len2 = torch.zeros(1, dtype=torch.int64, device="cuda")

    def split_call(items, flags):
        shb.sz_decompress_split_batch(items, 1, chunks, SEG, max_segments, d_len2, d_status, d_bad, d_result, flags=flags, d_scratch=split_scratch)

    d_chunks = torch.empty(32 * chunks, dtype=torch.uint8, device="cuda")
    d_descs = torch.empty(40, dtype=torch.uint8, device="cuda")
    d_istatus = torch.empty(1, dtype=torch.int32, device="cuda")
    d_iresult = torch.zeros(4, dtype=torch.int32, device="cuda")
    index_scratch = torch.empty(shb.sz_index_scratch_bytes(1, chunks, SEG, max_segments), dtype=torch.uint8, device="cuda")

    def index_call():
        shb.sz_index_batch(item_s, 1, chunks, SEG, max_segments, d_chunks, d_descs, d_istatus, d_iresult, d_scratch=index_scratch)

    # (a) the index against the sizing call
    split_call(item_s, 0)
    index_call()
    torch.cuda.synchronize()
    assert int(d_status[0]) == shb.RAW_DST_TOO_SMALL and int(d_len2[0]) == total and [int(x) for x in d_result.cpu().numpy()] == [0, 0, 1, 0]
    assert int(d_istatus[0]) == 0 and [int(x) for x in d_iresult.cpu().numpy()] == [chunks, 1, 1, 0]
    desc = d_descs.cpu().numpy().view(shb.SZ_DESC_DTYPE)[0]
    assert (int(desc["num_chunks"]), int(desc["total_len"])) == (chunks, total)
    recs = d_chunks.cpu().numpy().view(shb.SZ_CHUNK_DTYPE)
    assert (recs["dst_off"] == np.arange(chunks, dtype=np.uint64) * CL).all() and int(recs["ulen"].sum()) == total
    t_size, t_index = [], []
    for _ in range(REPS):
        t_size.append(once(lambda: split_call(item_s, 0)))
        t_index.append(once(index_call))
    a, b = stats(t_size), stats(t_index)
    emit(dict({"what": "index", "call": "split_sizing", "stream_bytes": total, "chunks": chunks, "segment_bytes": SEG, "reps": REPS}, **a))
    emit(dict({"what": "index", "call": "sz_index_batch", "stream_bytes": total, "chunks": chunks, "segment_bytes": SEG, "reps": REPS,
               "vs_split_sizing_min": round(b["ms_min"] / a["ms_min"], 4)}, **b))

    # ---- the container ----
    ws = shb.CompressWorkspace(total, CL)
    d_stream = torch.empty(ws.stream_capacity(total) + 16, dtype=torch.uint8, device="cuda")
    shb.compress_blocks(d_in, total, ws)
    shb.compact(total, ws, d_stream)
    stream_len = int(ws.stream_len.item())
    del ws
    _, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
    nb = shb.num_blocks(total, bs)
    d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    cdescs = shb.make_stream_descs([dict(stream=d_stream, stream_len=stream_len, block_offsets=d_boff, result=d_res, total_len=total, block_size=bs,
                                         header_len=hdr, num_blocks=nb)])
    shb.index_streams(cdescs, 1)
    assert [int(x) for x in d_res.cpu().numpy()] == [0, nb]

    # (b) the ranges
    counts = (1 << 10, 8 << 10, 64 << 10) if not args.only_small else (256, 1024)
    lengths = (4 << 10, 64 << 10, 1 << 20)
    max_count = max(counts)
    rscratch = torch.empty(shb.sz_decompress_ranges_scratch_bytes(max_count), dtype=torch.uint8, device="cuda")
    cscratch = torch.empty(shb.decompress_ranges_scratch_bytes(CL, max_count), dtype=torch.uint8, device="cuda")
    for length in lengths:
        for count in counts:
            cell = {"what": "ranges", "ranges": count, "range_bytes": length, "reps": REPS}
            if count * length > args.max_dst_gib * GIB:
                emit(dict(cell, call="not run", why="destinations of %d GiB exceed --max-dst-gib" % (count * length >> 30)))
                continue
            rng = np.random.default_rng(count + length)
            offs = rng.integers(0, total - length + 1, count).astype(np.int64)
            d_dst = torch.empty(count * length, dtype=torch.uint8, device="cuda")
            d_ranges = shb.make_ranges([(0, int(o), length, d_dst.data_ptr() + i * length) for i, o in enumerate(offs)])
            d_rstatus = torch.empty(count, dtype=torch.int32, device="cuda")
            d_rbad = torch.empty(count, dtype=torch.int32, device="cuda")
            variants = [
                ("sz_ranges", lambda: shb.sz_decompress_ranges(d_descs, 1, d_ranges, count, d_rstatus, d_rbad, d_scratch=rscratch)),
                ("sz_ranges_no_verify",
                 lambda: shb.sz_decompress_ranges(d_descs, 1, d_ranges, count, d_rstatus, d_rbad, flags=shb.SZ_NO_VERIFY, d_scratch=rscratch)),
                ("container_ranges", lambda: shb.decompress_ranges(cdescs, 1, d_ranges, count, d_rstatus, CL, cscratch)),
                ("split_full", lambda: split_call(item_d, 0)),
                ("split_full_no_verify", lambda: split_call(item_d, shb.SZ_NO_VERIFY)),
            ]
            sample = np.linspace(0, count - 1, 64).astype(np.int64)
            for name, call in variants:                    # warm-up, verified
                d_dst.fill_(0xA5)
                d_rstatus.fill_(0x55)
                call()
                torch.cuda.synchronize()
                if name.startswith("split"):
                    assert int(d_status[0]) == 0 and torch.equal(plain, d_in[:total]), name
                    continue
                assert int((d_rstatus != 0).sum().item()) == 0, name
                for i in sample:
                    assert torch.equal(d_dst[i * length:(i + 1) * length], d_in[int(offs[i]):int(offs[i]) + length]), (name, int(i))
            times = {name: [] for name, _ in variants}
            for _ in range(REPS):
                for name, call in variants:
                    times[name].append(once(call))
            s = {name: stats(t) for name, t in times.items()}
            for name, _ in variants:
                row = dict(cell, call=name, GBps_at_min=round(count * length / s[name]["ms_min"] / 1e6, 2), **s[name])
                if name.startswith("sz_ranges"):
                    row["vs_container_ranges_min"] = round(s[name]["ms_min"] / s["container_ranges"]["ms_min"], 4)
                    full = "split_full" if name == "sz_ranges" else "split_full_no_verify"
                    row["vs_split_full_min"] = round(s[name]["ms_min"] / s[full]["ms_min"], 4)
                emit(row)
            del d_dst, d_ranges
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
