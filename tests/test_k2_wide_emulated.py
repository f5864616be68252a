"""The wide block decoder (csrc/snappy_k2_wide.hpp: a workgroup per block) on the CPU wave emulator, held to K2 itself and to
the oracle.  Every job is decoded twice in a child process that names the job before it starts it -- by the emulated
k2_decode_block (emu_lib.decompress_block) and by k2_wide_kernel between inaccessible pages -- and the two must agree: the same
status, the same bytes where it is OK.  The result words are exact (k2_wide_cases.expected_result: blocks within the limits
that K2 accepts / blocks beyond the limits / blocks within the limits that K2 rejects / 0), so a fallback cannot hide a broken
wide path.  The wide call's own output is never a yardstick.

The emulator runs a workgroup of 16 wavefronts as 1,024 fibers, and a block the serial decoder takes costs it sixteen times
what it costs K2's one wavefront.  So the jobs of a kind are dealt over child processes that run side by side, and each job
runs at ONE workgroup size: job k of a kind at W = 16 when k is even, at W = 2 when it is odd, the other way round for the
hand-built blocks of k2_wide_cases, which also run at both sizes where they are cheap (see _CHILD).

The generated blocks of k2_wide_cases (the boundary, window, chain, bound and limit cases that tests/test_k2_wide_model.py holds
to their coverage conditions) are small, so they run at ALL FOUR workgroup sizes, and have a third yardstick: the model's
verdict, bytes and result words (see _MODEL_CHILD)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))

_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import emu_lib as emu, emu_k2_wide_lib as wide, k2_window_cases as kc, k2_wide_cases as wc
kind, count, part, parts = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
jobs = {"intact": kc.intact_jobs, "hand": kc.hand_jobs, "damaged": lambda: kc.damaged_jobs(count), "wide": wc.hand_jobs}[kind]()
assert wide.max_csz() == wc.WIDE_MAX_CSZ
problems, accepted, wide_path = [], 0, 0
for k, job in enumerate(jobs):
    if k % parts != part:
        continue
    name, stream, at, out_len = job
    sizes = wc.WAVES if kind == "wide" and out_len <= 4096 else (wc.WAVES[(k + (kind != "wide")) % 2],)
    print("job", name, flush=True)
    k2_st, k2_out = emu.decompress_block(stream, at, out_len)
    for waves in sizes:
        st, out, res = wide.decompress_block_wide(stream, at, out_len, waves)
        p = kc.check_job(job, st, out)                                   # the oracle
        if p is None and st != k2_st:
            p = "%s: status %d, K2's is %d" % (name, st, k2_st)
        if p is None and st == 0 and out != k2_out:
            p = name + ": bytes differ from K2's"
        if p is None and st != 0 and wc.must_accept(job):
            p = name + ": a valid block was rejected"
        want = wc.expected_result([(wc.within(stream, at, out_len), k2_st)])
        if p is None and res != want:
            p = "%s: result words %r, expected %r" % (name, res, want)
        if p:
            problems.append("W=%d %s" % (waves, p))
        accepted += st == 0
        wide_path += res[0]
print("jobs", len(jobs), "accepted", accepted, "wide", wide_path)
for p in problems:
    print("PROBLEM", p)
print("ok" if not problems else "failed")
"""


def _run(kind, count=0, env=None):
    """the jobs of a kind dealt over WORKERS children -> (accepted, decoded by the wide path)"""
    full_env = dict(os.environ, **(env or {}))
    import emu_lib
    import emu_k2_wide_lib
    emu_lib.lib(), emu_k2_wide_lib.lib()                       # built once, before the children want them
    kids = [subprocess.Popen([sys.executable, "-c", _CHILD, HERE, kind, str(count), str(part), str(WORKERS)], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, env=full_env) for part in range(WORKERS)]
    accepted = wide_path = 0
    failures = []
    for kid in kids:
        stdout, stderr = kid.communicate(timeout=3000)
        lines = stdout.strip().splitlines()
        last_job = next((ln for ln in reversed(lines) if ln.startswith("job ")), "none")
        problems = [ln for ln in lines if ln.startswith("PROBLEM")]
        if kid.returncode != 0:
            failures.append(("the emulator ended with status %d (negative: a signal, i.e. an access outside a guarded buffer) on %s"
                             % (kid.returncode, last_job), stderr[-1500:]))
        elif not lines or lines[-1] != "ok":
            failures.append((problems[:10], lines[-3:]))
        else:
            words = lines[-2].split()
            accepted += int(words[3])
            wide_path += int(words[5])
    assert not failures, failures
    return accepted, wide_path


def test_intact_blocks_take_the_wide_path_with_k2s_bytes():
    """Flavours 0-3 x block sizes 64, 700, 4097, 32768, 65535: every block accepted; every block of at most 32,768 bytes is
    decoded by the wide path itself ([0]), the 65,535-byte ones go serial ([1])."""
    import k2_window_cases as kc
    import k2_wide_cases as wc
    accepted, wide_path = _run("intact")
    jobs = kc.intact_jobs()
    assert accepted == len(jobs) >= 60
    assert wide_path == sum(1 for j in jobs if j[3] <= wc.WIDE_MAX_BLOCK) > 0


def test_hand_made_blocks_at_the_output_bound_as_k2_judges_them():
    accepted, wide_path = _run("hand")
    assert accepted > 0 and wide_path > 0


def test_damaged_blocks_get_k2s_verdict():
    """300 damaged element streams: what K2 rejects the wide path does not prove ([2]), what K2 still accepts it decodes."""
    accepted, wide_path = _run("damaged", 300)
    assert wide_path == accepted


def test_hand_built_blocks_aimed_at_the_shares_the_resolve_and_the_doubling():
    """k2_wide_cases.hand_bodies: empty shares, out_len 1 / 63 / 64 / 65 / 32768, literals that straddle a share boundary (the
    next entry at byte 63 of a share, behind its first 64 bytes, behind whole shares), the deepest copy chain, a copy offset of
    exactly op and of op + 1, overlapping copies, 22 copies in one window, all four element types, a valid block beyond the csz
    limit, size words and payloads that leave the stream."""
    accepted, wide_path = _run("wide")
    assert accepted > 0 and wide_path > 0


def test_hand_built_blocks_with_the_wavefronts_interleaved_at_random():
    """the same under EMU_SHUFFLE: the fibers of a pass in random order, whole wavefronts in bursts"""
    _run("wide", env={"EMU_SHUFFLE": "20261"})


_CONTAINERS = """
import sys
sys.path.insert(0, sys.argv[1])
import emu_lib as emu, emu_k2_wide_lib as wide, k2_wide_cases as wc, oracle_lib as oracle
part, parts = int(sys.argv[2]), int(sys.argv[3])
conts = wc.containers() + [wc.serial_container()]
for k, (name, stream, plain, offs, total, bs) in enumerate(conts):
    if k % parts != part:
        continue
    print("job", name, flush=True)
    hdr = oracle.read_header(stream)[2]
    k2_st, k2_out = emu.decompress(stream, total, bs, hdr)
    assert k2_st == 0 and k2_out == plain, name
    for waves, grid in ((wc.WAVES[k % 2], 3), (wc.WAVES[(k + 1) % 2], 1)):
        if grid == 1 and total > 40000:
            continue                                                      # (the large ones once: the emulator's time)
        rc, st, out, res = wide.decompress_wide(stream, offs, total, bs, waves, grid)
        assert rc == 0 and st == [0] * len(offs), (name, waves, grid, rc, st)
        assert out == plain, (name, waves, grid)
        assert res == ([len(offs), 0, 0, 0] if bs <= wc.WIDE_MAX_BLOCK else [0, len(offs), 0, 0]), (name, waves, grid, res)
print("ok")
"""


def test_whole_containers_plaintext_exact_and_every_block_on_the_wide_path():
    """terror2, alice, coding and element streams of flavours 0-3 at block sizes 700, 4,097 and 32,768 (last block partial),
    decoded whole by 3 workgroups and by 1, W = 2 and 16: all OK, the plaintext exact, [0] = the block count; a container at
    block size 65,535 goes serial block by block ([1])."""
    import emu_lib
    import emu_k2_wide_lib
    emu_lib.lib(), emu_k2_wide_lib.lib()
    kids = [subprocess.Popen([sys.executable, "-c", _CONTAINERS, HERE, str(part), str(WORKERS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True) for part in range(WORKERS)]
    failures = []
    for kid in kids:
        stdout, stderr = kid.communicate(timeout=3000)
        if kid.returncode != 0 or not stdout.strip().endswith("ok"):
            failures.append((kid.returncode, stdout[-300:], stderr[-1500:]))
    assert not failures, failures


_MODEL_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import emu_lib as emu, emu_k2_wide_lib as wide, k2_window_cases as kc, k2_wide_cases as wc
kind, part, parts = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
blocks = {"small": wc.small_blocks, "large": wc.large_blocks,
          "sweeps": lambda: [b for w in wc.ALL_WAVES for b in wc.boundary_blocks(w)] + wc.window_blocks()}[kind]()
jobs = wc.block_jobs(blocks)
problems, runs = [], 0
for k, (job, block) in enumerate(zip(jobs, blocks)):
    if k % parts != part:
        continue
    name, stream, at, out_len = job
    sizes = wc.ALL_WAVES if kind == "small" else ((block[3],) if block[3] else (wc.ALL_WAVES[k % 4],))
    print("job", name, flush=True)
    k2_st, k2_out = emu.decompress_block(stream, at, out_len)
    for waves in sizes:
        m = wc.job_model(job, waves)
        st, out, res = wide.decompress_block_wide(stream, at, out_len, waves)
        p = kc.check_job(job, st, out)                                   # the oracle
        if p is None and st != k2_st:
            p = "%s: status %d, K2's is %d" % (name, st, k2_st)
        if p is None and st == 0 and out != k2_out:
            p = name + ": bytes differ from K2's"
        if p is None and st != (0 if m.valid else 1):
            p = "%s: status %d, the model says valid = %r" % (name, st, m.valid)
        if p is None and st == 0 and out != m.out:
            p = name + ": bytes differ from the model's"
        if p is None and not (res == m.words == wc.expected_result([(wc.within(stream, at, out_len), k2_st)])):
            p = "%s: result words %r, the model's %r" % (name, res, m.words)
        if p:
            problems.append("W=%d %s" % (waves, p))
        runs += 1
print("runs", runs)
for p in problems:
    print("PROBLEM", p)
print("ok" if not problems else "failed")
"""

_TRIPS = """
import sys
sys.path.insert(0, sys.argv[1])
import emu_lib as emu, emu_k2_wide_lib as wide, k2_wide_cases as wc
part, parts = int(sys.argv[2]), int(sys.argv[3])
cases = [(t, waves) for t in wc.trips() for waves in (2, 16)]
for k, ((name, stream, offs, total, bs, blocks), waves) in enumerate(cases):
    if k % parts != part:
        continue
    print("job", name, waves, flush=True)
    models = [wc.model(body, n, waves) for body, n in blocks]
    rc, st, out, res = wide.decompress_wide(stream, offs, total, bs, waves, 1)          # ONE workgroup meets every block in turn
    assert rc == 0 and st == [0 if m.valid else 1 for m in models], (name, waves, rc, st)
    assert res == [sum(m.words[i] for m in models) for i in range(4)], (name, waves, res)
    for b, m in enumerate(models):
        k2_st, k2_out = emu.decompress_block(stream, offs[b], m.out_len)
        assert k2_st == st[b], (name, waves, b)
        if m.valid:
            assert out[b * bs:b * bs + m.out_len] == m.out == k2_out, (name, waves, b)
print("ok")
"""


def _children(script, args, env=None):
    """`script` in WORKERS children, each a part of the jobs -> their stdout lines; a child that died names its last job"""
    import emu_lib
    import emu_k2_wide_lib
    emu_lib.lib(), emu_k2_wide_lib.lib()
    kids = [subprocess.Popen([sys.executable, "-c", script, HERE] + args + [str(part), str(WORKERS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, env=dict(os.environ, **(env or {}))) for part in range(WORKERS)]
    failures, outputs = [], []
    for kid in kids:
        stdout, stderr = kid.communicate(timeout=3000)
        lines = stdout.strip().splitlines()
        last_job = next((ln for ln in reversed(lines) if ln.startswith("job ")), "none")
        if kid.returncode != 0:
            failures.append(("status %d (negative: a signal, i.e. an access outside a guarded buffer) on %s" % (kid.returncode, last_job),
                             stderr[-1500:]))
        elif not lines or lines[-1] != "ok":
            failures.append(([ln for ln in lines if ln.startswith("PROBLEM")][:10], lines[-3:]))
        outputs.append(lines)
    assert not failures, failures
    return outputs


def _runs(outputs):
    return sum(int(ln.split()[1]) for lines in outputs for ln in lines if ln.startswith("runs "))


def test_generated_small_blocks_at_all_four_workgroup_sizes_against_k2_the_oracle_and_the_model():
    """k2_wide_cases.small_blocks -- every element kind at every distance from the first, a middle and the last share boundary,
    entries at every offset, shares passed over, run-ons from every tag lane, copy chains in and across shares, the output bound
    per share -- each at W = 2, 4, 8 and 16: status and bytes are K2's, the oracle's and the model's, the result words the
    model's"""
    import k2_wide_cases as wc
    assert _runs(_children(_MODEL_CHILD, ["small"])) == 4 * len(wc.small_blocks())


def test_generated_large_blocks_the_limits_and_the_deepest_chains():
    """csz 0, 38,400 and 38,401, a run-on literal that ends at out_len 32,768, chains of 13 to 15 rounds: one W each"""
    import k2_wide_cases as wc
    assert _runs(_children(_MODEL_CHILD, ["large"])) == len(wc.large_blocks())


def test_boundary_and_window_sweeps_with_the_wavefronts_interleaved_at_random():
    """the two sweeps once more under EMU_SHUFFLE, each block at the workgroup size it is aimed at"""
    assert _runs(_children(_MODEL_CHILD, ["sweeps"], env={"EMU_SHUFFLE": "20262"})) > 3000


def test_trips_one_workgroup_meets_every_block_of_a_container_in_turn():
    """k2_wide_cases.trips at W = 2 and 16, grid 1: after a block that entered many shares one whose chain passes over them, a
    damaged block, valid ones; after a full 32 KiB block a tiny one.  Statuses, bytes and the summed result words are the
    model's: a control word, table entry, srcmap entry or staged byte left over from the trip before would show."""
    _children(_TRIPS, [])
