#!/usr/bin/env python3
"""Rates of the Snappy framing format on the device (snappy_hip_sz_compress_batch / snappy_hip_sz_decompress_batch /
snappy_hip_crc32c_batch) on a resident 1 GiB Silesia-mix carved into .sz streams: 8,192 items of 64 KiB,
1,024 of 1 MiB and one of 1 GiB, at chunks of 32 KiB.  Each call is timed with HIP events around it (one warm-up call, best of
three; the 1 GiB item once) and every result is verified: all items OK, the decoded bytes equal the source, sampled CRCs equal
a Python table walk.  Timed per batch:
  compress; decode with and without SNAPPY_HIP_SZ_NO_VERIFY; the sizing call (capacities of 0: the first walk of the chunk
  chains by sz_index_kernel, the plan and three launches that find nothing to do -- the decode call walks every chain twice);
  snappy_hip_crc32c_batch over the plaintext chunks, in GB/s.
Yardsticks in the same run, code the library had before: snappy_hip_raw_compress_batch over the same items at the same block
size, and snappy_hip_raw_decompress_batch over the same chunks as separate items (each chunk's plaintext as a raw stream of
its own, made by snappy_hip_raw_compress_batch).  One JSON line per measurement.
SNAPPY_HIP_CRC_TABLES=1 in the environment runs the CRC by a 256-entry byte table instead of slicing-by-4; --crc-only then
skips what does not depend on it.
Usage: python tools/sz_rate.py [--crc-only] [--out FILE]
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

GIB, CL = 1 << 30, 32768
POLY = 0x82F63B78


def crc32c(data):
    table = []
    for b in range(256):
        c = b
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
        table.append(c)
    c = 0xffffffff
    for b in data:
        c = (c >> 8) ^ table[(c ^ b) & 0xff]
    return c ^ 0xffffffff


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
    ap.add_argument("--crc-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    with open(os.path.join(silesia_mix.GOLDEN, "xml.snappy"), "rb") as f:
        st, d_xml = shb.decompress_resident(torch.from_numpy(np.frombuffer(f.read(), dtype=np.uint8).copy()).cuda())
    assert st == 0 and hashlib.sha256(d_xml.cpu().numpy().tobytes()).hexdigest() == silesia_mix.XML_TXT_SHA256
    unit = torch.from_numpy(silesia_mix.build_unit(d_xml.cpu().numpy(), seed=0).copy()).cuda()
    d_in = silesia_mix.container_from_unit(unit, GIB)
    rows = []
    tables = os.environ.get("SNAPPY_HIP_CRC_TABLES", "default")

    def emit(row):
        row["crc_tables"] = tables
        rows.append(row)
        print(json.dumps(row), flush=True)

    def batch(size, count, label):
        one = count == 1                                     # (one wavefront walks the one chain: one timed call, no warm-up)
        reps = 1 if one else 3
        per_item = (size + CL - 1) // CL
        chunks = count * per_item
        bound = max(shb.sz_compress_bound(size, CL), shb.raw_compress_bound(size, CL))      # (the raw yardstick writes to the same outputs)
        rng = np.random.default_rng(size + count)
        offs = rng.integers(0, GIB - size + 1, count).astype(np.int64) if not one else np.zeros(1, dtype=np.int64)
        comp = torch.empty(count * bound, dtype=torch.uint8, device="cuda")
        plain = torch.empty(count * size, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(max(shb.sz_compress_scratch_bytes(CL, count, chunks), shb.raw_compress_scratch_bytes(CL, chunks, chunks)),
                              dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(count, dtype=torch.int64, device="cuda")
        d_status = torch.empty(count, dtype=torch.int32, device="cuda")
        d_bad = torch.empty(count, dtype=torch.int32, device="cuda")
        d_result = torch.zeros(2, dtype=torch.int32, device="cuda")
        items_c = shb.make_raw_items([(d_in.data_ptr() + int(o), size, comp.data_ptr() + i * bound, bound) for i, o in enumerate(offs)])
        row = {"what": label, "item_bytes": size, "items": count, "chunk_len": CL, "chunks": chunks}
        nbytes = count * size

        def do_compress():
            shb.sz_compress_batch(items_c, count, CL, chunks, d_len, d_status, d_result, scratch)
        if not one:
            do_compress()
        t_c = timed(do_compress, reps)
        assert [int(x) for x in d_result.cpu().numpy()] == [chunks, count] and int((d_status != 0).sum().item()) == 0
        lens = d_len.cpu().numpy().copy()
        row.update(compressed_bytes=int(lens.sum()), compress_ms=round(t_c * 1e3, 3), compress_GBps=round(nbytes / t_c / 1e9, 2))

        if not args.crc_only:
            def do_raw_compress():
                shb.raw_compress_batch(items_c, count, CL, chunks, d_len, d_status, d_result, scratch)
            if not one:
                do_raw_compress()
            t_rc = timed(do_raw_compress, reps)
            assert int((d_status != 0).sum().item()) == 0
            row.update(raw_compress_ms=round(t_rc * 1e3, 3), raw_compress_GBps=round(nbytes / t_rc / 1e9, 2), compress_vs_raw_compress=round(t_rc / t_c, 3))
            do_compress()                                    # (the .sz streams again: the yardstick wrote over them)
            torch.cuda.synchronize()

        items_d = shb.make_raw_items([(comp.data_ptr() + i * bound, int(lens[i]), plain.data_ptr() + i * size, size) for i in range(count)])
        d_len2 = torch.zeros(count, dtype=torch.int64, device="cuda")
        dscratch = torch.empty(max(shb.sz_decompress_scratch_bytes(count, chunks), 256), dtype=torch.uint8, device="cuda")

        def verify_plain(what):
            assert int((d_status != 0).sum().item()) == 0 and int((d_len2 != size).sum().item()) == 0, what
            assert [int(x) for x in d_result.cpu().numpy()] == [chunks, count], what
            if one:
                assert torch.equal(plain, d_in[int(offs[0]):int(offs[0]) + size]), what
                return
            src = torch.from_numpy(offs).cuda()
            view = plain.view(count, size)
            step = max(1, (64 << 20) // size)
            ar = torch.arange(size, device="cuda")
            for lo in range(0, count, step):
                assert torch.equal(view[lo:lo + step], d_in[src[lo:lo + step, None] + ar[None, :]]), (what, lo)

        for flags, key in ((0, "decode"), (shb.SZ_NO_VERIFY, "decode_no_verify")):
            def do_decode():
                shb.sz_decompress_batch(items_d, count, chunks, d_len2, d_status, d_bad, d_result, flags=flags, d_scratch=dscratch)
            if not one:
                do_decode()
            t = timed(do_decode, reps, before=lambda: plain.fill_(0xA5))
            verify_plain(key)
            row.update({key + "_ms": round(t * 1e3, 3), key + "_GBps": round(nbytes / t / 1e9, 2)})
            if args.crc_only:
                break
        if not args.crc_only:
            row["verify_costs"] = round(row["decode_ms"] / row["decode_no_verify_ms"] - 1, 4)
            items_s = shb.make_raw_items([(comp.data_ptr() + i * bound, int(lens[i]), 0, 0) for i in range(count)])

            def do_size():
                shb.sz_decompress_batch(items_s, count, chunks, d_len2, d_status, d_bad, d_result, d_scratch=dscratch)
            if not one:
                do_size()
            t_s = timed(do_size, reps)
            assert int((d_status != shb.RAW_DST_TOO_SMALL).sum().item()) == 0 and int((d_len2 != size).sum().item()) == 0
            row.update(sizing_call_ms=round(t_s * 1e3, 3), chunk_headers_per_s=round(chunks / t_s))

        # the plaintext chunks as separate items: the CRC alone, and the raw decode yardstick
        starts = (offs[:, None] + (np.arange(per_item, dtype=np.int64) * CL)[None, :]).reshape(-1)
        sizes = np.minimum(CL, size - (np.arange(per_item, dtype=np.int64) * CL))
        sizes = np.tile(sizes, count)
        d_crc = torch.zeros(chunks, dtype=torch.int32, device="cuda")
        items_crc = shb.make_crc_items([(d_in.data_ptr() + int(s), int(n)) for s, n in zip(starts, sizes)])

        def do_crc():
            shb.crc32c_batch(items_crc, chunks, d_crc)
        do_crc()
        t_crc = timed(do_crc, 3)
        got = d_crc.cpu().numpy()
        for k in (0, chunks // 2, chunks - 1):
            want = crc32c(d_in[int(starts[k]):int(starts[k]) + int(sizes[k])].cpu().numpy().tobytes())
            assert int(got[k]) & 0xffffffff == want, (label, k)
        row.update(crc32c_batch_ms=round(t_crc * 1e3, 3), crc32c_batch_GBps=round(nbytes / t_crc / 1e9, 2))

        if not args.crc_only:
            rbound = shb.raw_compress_bound(CL, CL)
            del comp
            rcomp = torch.empty(chunks * rbound, dtype=torch.uint8, device="cuda")
            r_len = torch.zeros(chunks, dtype=torch.int64, device="cuda")
            r_status = torch.empty(chunks, dtype=torch.int32, device="cuda")
            items_rc = shb.make_raw_items([(d_in.data_ptr() + int(s), int(n), rcomp.data_ptr() + k * rbound, rbound)
                                           for k, (s, n) in enumerate(zip(starts, sizes))])
            shb.raw_compress_batch(items_rc, chunks, CL, chunks, r_len, r_status, d_result, scratch)
            assert int((r_status != 0).sum().item()) == 0
            rl = r_len.cpu().numpy()
            dst_at = (np.arange(count, dtype=np.int64) * size)[:, None] + (np.arange(per_item, dtype=np.int64) * CL)[None, :]
            dst_at = dst_at.reshape(-1)
            items_rd = shb.make_raw_items([(rcomp.data_ptr() + k * rbound, int(rl[k]), plain.data_ptr() + int(dst_at[k]), int(sizes[k]))
                                           for k in range(chunks)])
            r_len2 = torch.zeros(chunks, dtype=torch.int64, device="cuda")

            def do_raw_decode():
                shb.raw_decompress_batch(items_rd, chunks, r_len2, r_status)
            do_raw_decode()
            t_rd = timed(do_raw_decode, 3, before=lambda: plain.fill_(0xA5))
            assert int((r_status != 0).sum().item()) == 0
            d_status.zero_()
            d_len2.fill_(size)
            d_result.copy_(torch.tensor([chunks, count], dtype=torch.int32))
            verify_plain("raw decode yardstick")
            row.update(raw_decode_chunks_ms=round(t_rd * 1e3, 3), raw_decode_chunks_GBps=round(nbytes / t_rd / 1e9, 2),
                       decode_vs_raw_decode=round(t_rd / (row["decode_ms"] / 1e3), 3),
                       decode_no_verify_vs_raw_decode=round(t_rd / (row["decode_no_verify_ms"] / 1e3), 3))
        emit(row)

    batch(64 << 10, 8192, "8192 x 64 KiB")
    batch(1 << 20, 1024, "1024 x 1 MiB")
    batch(GIB, 1, "1 x 1 GiB (one stream: one wavefront walks its chain)")
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
