#!/usr/bin/env python3
"""Where does a workgroup per block beat a wavefront per block?  snappy_hip_decompress_blocks (K2) beside
snappy_hip_decompress_blocks_wide at W = 4, 8 and 16 on the same resident stream and offsets, in the same run, at block size
32,768:
  * the terror2 golden (4 blocks);
  * the dickens-, mozilla- and spamfile-size stand-ins of pim-compression_amd/standins.py (312, 1,564 and 2,571 blocks);
  * one 1 GiB Silesia-mix container (32,768 blocks).
Each call is timed with HIP events around it: three warm-up calls, then the median of 21 repetitions.  K2 is timed five times
over that way; the spread of those five medians ((max - min) / min) is the yardstick's own run-to-run noise, and the wide form
is called faster on a case only where it wins over K2's best median by more than that spread.  Every result is verified: all
statuses OK, the bytes equal to the plaintext, the result words [blocks, 0, 0, 0].
One JSON line per case, also written to profiles/k2_wide_rate.jsonl (or --out FILE).
Usage: python tools/k2_wide_rate.py [--out FILE] [--skip-gib]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pim-compression_amd"))
import silesia_mix  # noqa: E402
import snappy_hip_binding as shb  # noqa: E402
import standins  # noqa: E402

GIB, BS = 1 << 30, 32768
WARMUP, REPS, K2_RUNS = 3, 21, 5


def median_ms(call):
    import torch
    for _ in range(WARMUP):
        call()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def measure(name, d_in, n):
    """d_in: the plaintext on the device (n bytes) -> one row"""
    import torch
    d_stream = shb.compress_resident(d_in, BS, n)
    stream_len = int(d_stream.numel())
    total, bs, hdr = shb.parse_header(bytes(d_stream[:10].cpu().numpy()))
    assert (total, bs) == (n, BS)
    nb = shb.num_blocks(total, bs)
    d_boff = torch.empty(nb, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int32, device="cuda")
    descs = shb.make_stream_descs([dict(stream=d_stream, stream_len=stream_len, block_offsets=d_boff, result=d_res, total_len=total,
                                        block_size=bs, header_len=hdr, num_blocks=nb)])
    shb.index_streams(descs, 1)
    assert [int(x) for x in d_res.cpu().numpy()] == [0, nb]
    d_out = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    d_status = torch.empty(nb, dtype=torch.int32, device="cuda")
    d_result = torch.empty(4, dtype=torch.int32, device="cuda")

    def k2():
        shb.decompress_blocks(d_stream, stream_len, d_boff, total, bs, d_out, d_status)

    def verified():
        torch.cuda.synchronize()
        return int((d_status != 0).sum().item()) == 0 and torch.equal(d_out[:n], d_in[:n])

    k2_runs = [median_ms(k2) for _ in range(K2_RUNS)]
    assert verified()
    k2_ms = min(k2_runs)
    spread = (max(k2_runs) - k2_ms) / k2_ms
    row = {"case": name, "blocks": nb, "plain_bytes": n, "stream_bytes": stream_len, "k2_ms_medians": [round(t, 4) for t in k2_runs],
           "k2_ms": round(k2_ms, 4), "k2_spread": round(spread, 4)}
    for waves in (4, 8, 16):
        d_out.zero_()
        d_status.fill_(7)

        def wide():
            shb.decompress_blocks_wide(d_stream, stream_len, d_boff, total, bs, d_out, d_status, d_result, waves)

        t = median_ms(wide)
        assert verified()
        words = [int(x) for x in d_result.cpu().numpy()]
        assert words == [nb, 0, 0, 0], words
        row["wide%d_ms" % waves] = round(t, 4)
        row["wide%d_result" % waves] = words[:3]
        row["wide%d_over_k2" % waves] = round(t / k2_ms, 4)
        row["wide%d_faster" % waves] = bool(t < k2_ms * (1 - spread))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k2_wide_rate.jsonl"))
    ap.add_argument("--skip-gib", action="store_true", help="leave the 1 GiB container out")
    args = ap.parse_args()
    import torch
    with open(os.path.join(silesia_mix.GOLDEN, "xml.snappy"), "rb") as f:
        st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(f.read(), dtype=np.uint8).copy()).cuda())
    xml_plain = d_xml.cpu().numpy().tobytes()
    assert st == 0 and hashlib.sha256(xml_plain).hexdigest() == silesia_mix.XML_TXT_SHA256
    texts = standins.prose_texts()
    cases = [("terror2", lambda: standins.golden_text("terror2.txt")), ("dickens-size", lambda: standins.dickens_like(texts)),
             ("mozilla-size", lambda: standins.mozilla_like(xml_plain)), ("spamfile-size", lambda: standins.spamfile_like(texts))]
    rows = []
    for name, make in cases:
        plain = make()
        d_in = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
        rows.append(measure(name, d_in, len(plain)))
        print(json.dumps(rows[-1]), flush=True)
        del d_in
    if not args.skip_gib:
        unit = torch.from_numpy(silesia_mix.build_unit(np.frombuffer(xml_plain, dtype=np.uint8), seed=0).copy()).cuda()
        d_in = silesia_mix.container_from_unit(unit, GIB)
        rows.append(measure("silesia-mix 1 GiB", d_in, GIB))
        print(json.dumps(rows[-1]), flush=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
