#!/usr/bin/env python3
"""The raw / .sz compress calls with a table workspace (snappy_hip_raw_compress_batch_tables, snappy_hip_sz_compress_batch_tables:
K1's global-table wavefronts) beside the base calls (K1's LDS-table form) on the same resident items in one process (DESIGN.md
3.15).  Items carved from a resident 1 GiB Silesia-mix:
  1,024 x 1 MiB at 32 KiB; 16,384 x 64 KiB at 32 KiB; one item of 1 GiB at 32 KiB; 1,024 x 1 MiB at 4 KiB (the filter-alone
  instances); 64 x 64 KiB at 32 KiB (the small-batch rule: both calls run the same fragment kernel).
Both formats.  Each call is timed with HIP events around it, as tools/sz_rate.py times: one warm-up call, then REPS calls, the
best taken; the base call -- unchanged code, the yardstick -- also reports its run-to-run spread over those calls,
(max - min) / min.  Every pair is verified: all items OK, lengths equal, every output byte equal, d_result[2] = the fragments
(0 under the small-batch rule).  One JSON line per pair, appended to profiles/items_gt_rate.jsonl.
Usage: python tools/items_gt_rate.py [--out FILE] [--reps N]
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

GIB = 1 << 30


def timed_all(call, reps):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "items_gt_rate.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    with open(os.path.join(silesia_mix.GOLDEN, "xml.snappy"), "rb") as f:
        st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(f.read(), dtype=np.uint8).copy()).cuda())
    assert st == 0 and hashlib.sha256(d_xml.cpu().numpy().tobytes()).hexdigest() == silesia_mix.XML_TXT_SHA256
    unit = torch.from_numpy(silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0).copy()).cuda()
    d_in = silesia_mix.container_from_unit(unit, GIB)
    d_tables = shb.compress_tables()
    props = torch.cuda.get_device_properties(0)
    device = {"name": props.name, "cus": props.multi_processor_count, "tables_bytes": d_tables.numel()}

    def pair(fmt, size, count, bs, label):
        reps = args.reps if size < GIB else 3
        per_item = (size + bs - 1) // bs
        units = count * per_item
        bound = (shb.raw_compress_bound if fmt == "raw" else shb.sz_compress_bound)(size, bs)
        need = (shb.raw_compress_scratch_bytes if fmt == "raw" else shb.sz_compress_scratch_bytes)(bs, count, units)
        base_call, new_call = (shb.raw_compress_batch, shb.raw_compress_batch_tables) if fmt == "raw" else (shb.sz_compress_batch, shb.sz_compress_batch_tables)
        rng = np.random.default_rng(size + count)
        offs = rng.integers(0, GIB - size + 1, count).astype(np.int64) if count > 1 else np.zeros(1, dtype=np.int64)
        out = [torch.empty(count * bound, dtype=torch.uint8, device="cuda") for _ in range(2)]
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        d_len = [torch.zeros(count, dtype=torch.int64, device="cuda") for _ in range(2)]
        d_status = [torch.full((count,), 0x55, dtype=torch.int32, device="cuda") for _ in range(2)]
        d_result = [torch.full((4,), 0x77, dtype=torch.int32, device="cuda") for _ in range(2)]
        items = [shb.make_raw_items([(d_in.data_ptr() + int(o), size, out[k].data_ptr() + i * bound, bound) for i, o in enumerate(offs)]) for k in range(2)]

        def do_base():
            base_call(items[0], count, bs, units, d_len[0], d_status[0], d_result[0], scratch)

        def do_new():
            new_call(items[1], count, bs, units, d_len[1], d_status[1], d_result[1], d_tables=d_tables, d_scratch=scratch)
        for k in range(2):
            out[k].fill_(0xEE)
        do_base()
        do_new()
        torch.cuda.synchronize()
        t_base = timed_all(do_base, reps)
        t_new = timed_all(do_new, reps)
        t_base += timed_all(do_base, reps)                   # (the yardstick on both sides of the new call)
        res = [[int(x) for x in r.cpu().numpy()] for r in d_result]
        assert int((d_status[0] != 0).sum().item()) == 0 and int((d_status[1] != 0).sum().item()) == 0, label
        assert res[0][:2] == res[1][:2] == [units, count] and res[1][2] in (0, units) and res[1][3] == 0, (label, res)
        assert torch.equal(d_len[0], d_len[1]) and torch.equal(out[0], out[1]), label
        nbytes = count * size
        row = {"what": label, "format": fmt, "item_bytes": size, "items": count, "block_size": bs, "fragments": units,
               "compressed_bytes": int(d_len[0].sum().item()), "reps": reps,
               "base_ms": round(min(t_base), 3), "base_ms_all": [round(t, 3) for t in t_base], "base_spread": round((max(t_base) - min(t_base)) / min(t_base), 4),
               "tables_ms": round(min(t_new), 3), "tables_ms_all": [round(t, 3) for t in t_new],
               "base_GBps": round(nbytes / min(t_base) / 1e6, 2), "tables_GBps": round(nbytes / min(t_new) / 1e6, 2),
               "tables_vs_base": round(min(t_base) / min(t_new), 3), "global_table_fragments": res[1][2], "device": device}
        print(json.dumps(row), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        del out, scratch
        torch.cuda.empty_cache()

    for fmt in ("raw", "sz"):
        pair(fmt, 1 << 20, 1024, 32768, "1024 x 1 MiB at 32 KiB")
        pair(fmt, 64 << 10, 16384, 32768, "16384 x 64 KiB at 32 KiB")
        pair(fmt, GIB, 1, 32768, "1 x 1 GiB at 32 KiB")
        pair(fmt, 1 << 20, 1024, 4096, "1024 x 1 MiB at 4 KiB")
        pair(fmt, 64 << 10, 64, 32768, "64 x 64 KiB at 32 KiB (small-batch rule)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
