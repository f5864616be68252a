#!/usr/bin/env python3
"""snappy_hip_sz_decompress_split_batch next to snappy_hip_sz_decompress_batch on the same batches in the same run (DESIGN.md
3.13): a resident 1 GiB Silesia-mix carved into .sz streams of 32 KiB chunks by snappy_hip_sz_compress_batch -- 8,192 items of
64 KiB, 1,024 of 1 MiB and one of 1 GiB.  Per batch: the sizing call (capacities of 0), the decode, and the decode with
SNAPPY_HIP_SZ_NO_VERIFY, by the base call and by the split call at segment_bytes of 256 KiB, 1 MiB and 4 MiB.  Every variant is
run once and verified (statuses, lengths, d_result, the decoded bytes against the source), then all variants are timed in turn,
REPS rounds, with HIP events around each call: the minimum, the median and the maximum are reported, and the base call's
(max - min) / min is the run-to-run spread the comparison is read against.  One JSON line per batch and variant.
Usage: python tools/sz_split_rate.py [--out FILE] [--only-small]
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

GIB, CL, REPS = 1 << 30, 32768, 7
SEGMENTS = (256 << 10, 1 << 20, 4 << 20)


def once(call):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-small", action="store_true", help="a 64 MiB source and batches scaled to it: a rehearsal")
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

    def batch(size, count, label):
        per_item = (size + CL - 1) // CL
        chunks = count * per_item
        bound = shb.sz_compress_bound(size, CL)
        rng = np.random.default_rng(size + count)
        offs = rng.integers(0, total - size + 1, count).astype(np.int64) if count > 1 else np.zeros(1, dtype=np.int64)
        comp = torch.empty(count * bound, dtype=torch.uint8, device="cuda")
        plain = torch.empty(count * size, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(count, dtype=torch.int64, device="cuda")
        d_status = torch.empty(count, dtype=torch.int32, device="cuda")
        d_bad = torch.empty(count, dtype=torch.int32, device="cuda")
        d_result = torch.zeros(4, dtype=torch.int32, device="cuda")
        cscratch = torch.empty(shb.sz_compress_scratch_bytes(CL, count, chunks), dtype=torch.uint8, device="cuda")
        items_c = shb.make_raw_items([(d_in.data_ptr() + int(o), size, comp.data_ptr() + i * bound, bound) for i, o in enumerate(offs)])
        shb.sz_compress_batch(items_c, count, CL, chunks, d_len, d_status, d_result, cscratch)
        assert int((d_status != 0).sum().item()) == 0
        lens = d_len.cpu().numpy().copy()
        del cscratch
        items_d = shb.make_raw_items([(comp.data_ptr() + i * bound, int(lens[i]), plain.data_ptr() + i * size, size) for i in range(count)])
        items_s = shb.make_raw_items([(comp.data_ptr() + i * bound, int(lens[i]), 0, 0) for i in range(count)])
        d_len2 = torch.zeros(count, dtype=torch.int64, device="cuda")
        base_scratch = torch.empty(max(shb.sz_decompress_scratch_bytes(count, chunks), 256), dtype=torch.uint8, device="cuda")

        def check(what, sizing, large):
            """the verdicts of the call that just ran; large: None for the base call, else the items of more than one segment"""
            want = shb.RAW_DST_TOO_SMALL if sizing else 0
            assert int((d_status != want).sum().item()) == 0 and int((d_len2 != size).sum().item()) == 0, what
            res = [int(x) for x in d_result.cpu().numpy()]
            assert res[:2] == ([0, 0] if sizing else [chunks, count]), (what, res)
            if large is not None:
                assert res[2:] == [large, 0], (what, res)
            if sizing:
                return
            assert int((d_bad != -1).sum().item()) == 0, what
            if count == 1:
                assert torch.equal(plain, d_in[int(offs[0]):int(offs[0]) + size]), what
                return
            src = torch.from_numpy(offs).cuda()
            view = plain.view(count, size)
            step = max(1, (64 << 20) // size)
            ar = torch.arange(size, device="cuda")
            for lo in range(0, count, step):
                assert torch.equal(view[lo:lo + step], d_in[src[lo:lo + step, None] + ar[None, :]]), (what, lo)

        variants = []                                      # (call name, segment_bytes or None, kind, callable)
        for kind, items, flags in (("sizing", items_s, 0), ("decode", items_d, 0), ("decode_no_verify", items_d, shb.SZ_NO_VERIFY)):
            def base(items=items, flags=flags):
                shb.sz_decompress_batch(items, count, chunks, d_len2, d_status, d_bad, d_result, flags=flags, d_scratch=base_scratch)
            variants.append(("base", None, kind, base))
        scratches = {}
        for seg in SEGMENTS:
            max_segments = int(sum(-(-int(n) // seg) for n in lens))
            scratches[seg] = torch.empty(shb.sz_decompress_split_scratch_bytes(count, chunks, seg, max_segments), dtype=torch.uint8, device="cuda")
            for kind, items, flags in (("sizing", items_s, 0), ("decode", items_d, 0), ("decode_no_verify", items_d, shb.SZ_NO_VERIFY)):
                def split(items=items, flags=flags, seg=seg, max_segments=max_segments):
                    shb.sz_decompress_split_batch(items, count, chunks, seg, max_segments, d_len2, d_status, d_bad, d_result, flags=flags,
                                                  d_scratch=scratches[seg])
                variants.append(("split", seg, kind, split))
        for name, seg, kind, call in variants:             # warm-up, verified
            plain.fill_(0xA5)
            d_status.fill_(0x55)
            d_len2.zero_()
            call()
            torch.cuda.synchronize()
            check((label, name, seg, kind), kind == "sizing", None if seg is None else int((lens > seg).sum()))
        times = {(name, seg, kind): [] for name, seg, kind, _ in variants}
        for _ in range(REPS):
            for name, seg, kind, call in variants:
                if kind != "sizing":
                    plain.fill_(0xA5)
                times[(name, seg, kind)].append(once(call))
        nbytes = count * size
        for (name, seg, kind), t in times.items():
            t = sorted(t)
            base_t = sorted(times[("base", None, kind)])
            emit({"batch": label, "item_bytes": size, "items": count, "chunk_len": CL, "chunks": chunks, "compressed_bytes": int(lens.sum()),
                  "call": name, "segment_bytes": seg, "what": kind, "reps": REPS, "ms_min": round(t[0], 4), "ms_median": round(t[len(t) // 2], 4),
                  "ms_max": round(t[-1], 4), "GBps_at_min": round(nbytes / t[0] / 1e6, 2), "base_ms_min": round(base_t[0], 4),
                  "base_spread": round((base_t[-1] - base_t[0]) / base_t[0], 4), "vs_base_min": round(t[0] / base_t[0], 4)})

    if args.only_small:
        batch(64 << 10, 512, "512 x 64 KiB")
        batch(total, 1, "1 x 64 MiB")
    else:
        batch(64 << 10, 8192, "8192 x 64 KiB")
        batch(1 << 20, 1024, "1024 x 1 MiB")
        batch(GIB, 1, "1 x 1 GiB")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
