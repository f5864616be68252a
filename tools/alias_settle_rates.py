#!/usr/bin/env python3
"""Settles per window of K1's stream form under the CPU wave emulator, by data class of the benchmark's mix and by the size of
the duplicate analysis' tables (variant 43503: the global-table kernel, 256 slots; 3501: the LDS-table kernel, 512), with the
counters of the alias resolution (snappy_kernels.hpp: g_alias_stats).  About a minute per MiB.
    python tools/alias_settle_rates.py [KiB per class, default 256]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pim-compression_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import emu_k1_alias_lib as emu
import oracle_lib as oracle
import silesia_mix


def main():
    kib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    n = kib << 10
    with open(os.path.join(ROOT, "tests", "golden", "xml.snappy"), "rb") as f:
        st, xml = oracle.decompress(f.read())
    assert st == 0
    text = (silesia_mix._read("world192.txt").tobytes() + silesia_mix._read("plrabn12.txt").tobytes())[:n]
    classes = {"text": text, "xml": bytes(xml[256 << 10:(256 << 10) + n]), "records": silesia_mix._records(1 << 18, 2000).tobytes()[:n]}
    for name, data in classes.items():
        ref = oracle.compress(data, 32768)
        for cv in (43503, 3501):
            emu.stream_stats(), emu.alias_stats()
            same = emu.compress(data, 32768, cv) == ref
            s, a = emu.stream_stats(), emu.alias_stats()
            w = max(s[emu.WINDOWS_TAKEN], 1)
            print("%-8s variant %5d  same as the oracle %s  windows %6d  per window: settles %.3f  long way %.3f  long way finding nothing %.3f | "
                  % (name, cv, same, w, s[emu.SETTLES] / w, s[emu.LONG_WAY] / w, a[9] / w)
                  + "  ".join("%s %.3f" % (k, v / w) for k, v in zip(emu.ALIAS_STATS[:9], a)), flush=True)


if __name__ == "__main__":
    main()
