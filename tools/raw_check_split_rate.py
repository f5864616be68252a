#!/usr/bin/env python3
"""Rate of snappy_hip_raw_check_split_batch on ONE large raw stream.  A resident Silesia-mix is
raw-compressed at 32 KiB fragments (snappy_hip_raw_compress_batch, one item) in sizes of 64 MiB, 256 MiB and 1 GiB; the one
stream is checked by the split check at the default segment.  Each call is timed with HIP events around it: one warm-up call,
then three, of which the best and the spread (slowest - fastest) are reported; every run is verified: status OK, d_result =
[1, 0, 0, 0], out_len the plaintext's length.  Beside it, on the same item in the same run: the serial check
(snappy_hip_raw_check_batch, one wavefront) for the 64 MiB item only -- it takes hundreds of milliseconds -- and the split
decode (snappy_hip_raw_decompress_split_batch, units of 65,536, the same segment).  One more row: the 64 MiB item with ONE copy
offset, three quarters into the stream, set to 0; it falls back to the serial checker ([0, 0, 1, 0], INVALID) and its time is
recorded as it is.  One JSON line per measurement.
Usage: python tools/raw_check_split_rate.py [--sizes-mib 64,256,1024] [--out FILE]
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
from raw_split_rate import timed  # noqa: E402

MIB, BS, UNIT, SEGMENT = 1 << 20, 32768, 65536, 16384
OK, INVALID = 0, 1


def copy2_behind(stream, hdr, at_least):
    """position of the first 2-byte-offset copy at or behind compressed byte `at_least`: one walk over the elements"""
    at, n = hdr, len(stream)
    while at < n:
        tag = stream[at]
        t, v = tag & 3, tag >> 2
        if t == 0:
            nb = v - 59 if v >= 60 else 0
            at += 1 + nb + (int.from_bytes(stream[at + 1:at + 1 + nb], "little") if nb else v) + 1
        else:
            if t == 2 and at >= at_least:
                return at
            at += (2, 3, 5)[t - 1]
    raise SystemExit("no copy with a 2-byte offset behind byte %d" % at_least)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", default="64,256,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_check_split_rate.jsonl"))
    args = ap.parse_args()
    import torch
    sizes = [int(x) * MIB for x in args.sizes_mib.split(",")]
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
        bound = shb.raw_compress_bound(size, BS)
        frags = (size + BS - 1) // BS
        comp = torch.empty(bound, dtype=torch.uint8, device="cuda")
        plain = torch.empty(size + 16, dtype=torch.uint8, device="cuda")[:size]
        d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_status = torch.empty(1, dtype=torch.int32, device="cuda")
        d_result = torch.zeros(4, dtype=torch.int32, device="cuda")
        shb.raw_compress_batch(shb.make_raw_items([(d_in.data_ptr(), size, comp.data_ptr(), bound)]), 1, BS, frags, d_len, d_status, d_result[:2])
        assert int(d_status.item()) == OK
        clen = int(d_len.item())
        items = shb.make_raw_items([(comp.data_ptr(), clen, plain.data_ptr(), size)])
        d_len2 = torch.zeros(1, dtype=torch.int64, device="cuda")
        max_segments, max_units = clen // SEGMENT + 1, size // UNIT + 1

        def reset():
            d_status.fill_(0x55)
            d_len2.fill_(0)
            d_result.fill_(0x77)

        def verify(status=OK, result=None):
            assert (int(d_status.item()), int(d_len2.item())) == (status, size), (label, int(d_status.item()), int(d_len2.item()))
            if result:
                assert d_result.cpu().tolist() == result, (label, d_result.cpu().tolist())

        # ---- the split check ----
        scratch = torch.empty(shb.raw_check_split_scratch_bytes(1, SEGMENT, max_segments), dtype=torch.uint8, device="cuda")

        def do_check_split():
            shb.raw_check_split_batch(items, 1, SEGMENT, max_segments, d_len2, d_status, d_result, scratch)
        reset()
        do_check_split()
        verify(OK, [1, 0, 0, 0])
        t_split = timed(do_check_split, 3, before=reset, after=lambda: verify(OK, [1, 0, 0, 0]))
        emit({"what": "split check, " + label, "segment_bytes": SEGMENT, "compressed_bytes": clen, "max_segments": max_segments,
              "scratch_bytes": scratch.numel(), **ms(t_split), "GBps_compressed": round(clen / t_split[0] / 1e9, 2)})
        # ---- the split decode of the same item ----
        scratch_d = torch.empty(shb.raw_decompress_split_scratch_bytes(1, UNIT, SEGMENT, max_segments, max_units), dtype=torch.uint8, device="cuda")

        def do_decode_split():
            shb.raw_decompress_split_batch(items, 1, UNIT, SEGMENT, max_segments, max_units, d_len2, d_status, d_result, scratch_d)

        def verify_decode():
            verify(OK, [1, 0, 0, 0])
            assert torch.equal(plain, d_in[:size]), label
        reset()
        do_decode_split()
        verify_decode()
        t_decode = timed(do_decode_split, 3, before=lambda: (reset(), plain.fill_(0xA5)), after=verify_decode)
        emit({"what": "split decode, " + label, "segment_bytes": SEGMENT, "unit_len": UNIT, **ms(t_decode),
              "check_over_decode": round(t_split[0] / t_decode[0], 2)})
        del scratch_d
        if size == sizes[0]:
            # ---- the serial check (one wavefront) ----
            def do_serial():
                shb.raw_check_batch(items, 1, d_len2, d_status)
            reset()
            do_serial()
            verify()
            t_serial = timed(do_serial, 3, before=reset, after=verify)
            emit({"what": "serial check (raw_check_batch), " + label, **ms(t_serial)})
            emit({"what": "summary, " + label, "serial_over_split": round(t_serial[0] / t_split[0], 1),
                  # faster by more than the sum of the two spreads
                  "faster_beyond_spreads": bool(t_serial[0] - t_split[0] > (t_serial[-1] - t_serial[0]) + (t_split[-1] - t_split[0]))})
            # ---- one copy offset damaged: the item falls back ----
            host = comp[:clen].cpu().numpy().tobytes()
            hdr = next(k + 1 for k in range(5) if host[k] < 0x80)
            at = copy2_behind(host, hdr, 3 * clen // 4)
            keep = comp[at + 1:at + 3].clone()
            comp[at + 1:at + 3] = 0
            reset()
            do_check_split()
            verify(INVALID, [0, 0, 1, 0])
            t_bad = timed(do_check_split, 3, before=reset, after=lambda: verify(INVALID, [0, 0, 1, 0]))
            reset()
            do_serial()
            verify(INVALID)
            emit({"what": "split check of a damaged item (falls back), " + label, "damaged_at": at, **ms(t_bad)})
            comp[at + 1:at + 3] = keep
        del scratch, comp, plain
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
