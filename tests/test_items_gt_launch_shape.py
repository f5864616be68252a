"""csrc/launch_shape.hpp -- the grid of the raw / .sz compress calls that take a table workspace
(snappy_hip_raw_compress_batch_tables, snappy_hip_sz_compress_batch_tables): the smallest of max_fragments, the global-table
wavefronts the device holds, the tables of the workspace and SNAPPY_HIP_GT_WAVES when set; and the small-batch rule in front of
it.  Compiled on the CPU (no HIP) and compared, row by row, with the restatement below over a whole MI355X and a 32-CU
partition, workspaces from one table to the full grid, batches of 1, the small-batch threshold and one more, and the knob."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pim-compression_amd", "csrc")

SRC = r'''
#include <cstdio>
#include "launch_shape.hpp"
using namespace launch_shape;
int main() {
    unsigned cus, lds_wave, gt_wave, frags;
    unsigned long long tables_bytes;
    int forced;
    while (std::scanf("%u %u %u %u %llu %d", &cus, &lds_wave, &gt_wave, &frags, &tables_bytes, &forced) == 6) {
        DeviceShape d;
        d.cus = cus;
        K1Knobs k;
        k.lds_wave_bytes = lds_wave;
        k.gt_wave_bytes = gt_wave;
        k.waves_forced = forced;
        k.lds_waves_forced = 7;          // (the container's knob: no business of this launch)
        std::printf("%llu %u %d %u\n", (unsigned long long)items_gt_tables(tables_bytes), gt_wave_budget(d, k), (int)items_gt_small_batch(d, k, frags),
                    items_gt_grid(d, k, frags, tables_bytes));
    }
    return 0;
}
'''

LDS_PER_CU, SLOTS_PER_CU, TABLE = 160 << 10, 32, 65536


def alloc(n):
    return (n + 1023) & ~1023


def restated(cus, lds_wave, gt_wave, frags, tables_bytes, forced):
    """the issue's words, not the header's code"""
    tables = (tables_bytes - 256) // TABLE if tables_bytes > 256 else 0
    budget = min(SLOTS_PER_CU, LDS_PER_CU // alloc(gt_wave)) * cus
    resident = max(1, min(SLOTS_PER_CU, LDS_PER_CU // alloc(lds_wave))) * cus       # the base call's grid cap (update_resident_waves)
    small = forced <= 0 and frags <= resident
    grid = min(frags, budget, tables)
    if forced > 0:
        grid = min(grid, forced)
    return tables, budget, int(small), grid


def threshold(cus, lds_wave):
    return max(1, min(SLOTS_PER_CU, LDS_PER_CU // alloc(lds_wave))) * cus


def rows():
    out = []
    # (LDS of an LDS-table wavefront, static LDS of a global-table wavefront): 32 KiB blocks in the stream form behind the slot
    # cache; 4 KiB blocks in the bulk form behind the filter alone; 256-byte blocks
    for lds_wave, gt_wave in ((2 * 16384 + 4096, 6144), (2 * 4096 + 4096, 3072), (2 * 256 + 4096, 3072)):
        for cus in (256, 32):
            full = 256 + cus * SLOTS_PER_CU * TABLE
            t = threshold(cus, lds_wave)
            for tables_bytes in (256 + TABLE, 256 + 2 * TABLE - 1, 256 + 64 * TABLE, full // 2, full - 1, full, 2 * full):
                for frags in (1, t, t + 1, 3 * t, 1 << 20, 0xffffffff):
                    for forced in (-1, 0, 1, 64, 100000):
                        out.append((cus, lds_wave, gt_wave, frags, tables_bytes, forced))
    return out


def test_items_gt_grid_and_small_batch_rule_against_the_restatement(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(SRC)
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])
    cases = rows()
    out = subprocess.run([str(exe)], input="".join("%d %d %d %d %d %d\n" % r for r in cases), capture_output=True, text=True)
    assert out.returncode == 0
    got = [tuple(int(x) for x in ln.split()) for ln in out.stdout.strip().splitlines()]
    assert len(got) == len(cases) == 3 * 2 * 7 * 6 * 5
    wrong = [(c, g, restated(*c)) for c, g in zip(cases, got) if g != restated(*c)]
    assert not wrong, wrong[:5]


def test_the_figures_of_a_whole_mi355x_at_32_kib():
    """what the documents state: 26 global-table wavefronts per CU (160 KiB / 6 KiB) against 4 LDS-table ones (36 KiB each), so
    batches of up to 1,024 fragments stay with the LDS form; one table is one wavefront; the full workspace is not the limit"""
    lds_wave, gt_wave = 2 * 16384 + 4096, 6144
    full = 256 + 8192 * TABLE
    assert restated(256, lds_wave, gt_wave, 1024, full, -1) == (8192, 26 * 256, 1, 1024)
    assert restated(256, lds_wave, gt_wave, 1025, full, -1) == (8192, 26 * 256, 0, 1025)
    assert restated(256, lds_wave, gt_wave, 1 << 20, full, -1)[3] == 26 * 256
    assert restated(256, lds_wave, gt_wave, 1 << 20, 256 + TABLE, -1)[3] == 1
    assert restated(256, lds_wave, gt_wave, 512, full, 64) == (8192, 26 * 256, 0, 64)
    assert restated(32, lds_wave, gt_wave, 1 << 20, full, -1)[3] == 26 * 32
