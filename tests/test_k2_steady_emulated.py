"""The two window loops of k2_decode_block (csrc/snappy_kernels.hpp) on the CPU wave emulator: the blocks of
tests/k2_steady_cases.py -- compressed sizes around the first interior windows, at every alignment and with 0 to 200 bytes of
stream behind the block; literals that run on out of a steady window; defects in the first, a middle and the last steady
window -- each decoded ALONE into a buffer of exactly its output length between inaccessible pages, its stream in front of
one too.  A byte written outside the window or read behind the stream is a fault -- a legitimate failure here, so the decoding
runs in a child process that names the job it is on before it starts it."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import emu_lib as emu, emu_raw_lib as er, k2_steady_cases as sc
kind = sys.argv[2]
problems, accepted, rejected = [], 0, 0
if kind == "raw":
    items = sc.raw_items()
    for item in items:
        name, s, n = item
        print("job", name, flush=True)
        r, b = er.decompress([(s, n)], grid=1)
        p = "a kernel wrote in front of a window" if r != 0 else sc.judge_raw(item, int(b.status[0]), int(b.out_len[0]), b.window(0))
        if p:
            problems.append(p)
        accepted += int(b.status[0]) == 0
        rejected += int(b.status[0]) != 0
else:
    for job in {"hand": sc.hand_jobs, "intact": sc.intact_jobs}[kind]():
        name, stream, at, out_len = job
        print("job", name, flush=True)
        st, out = emu.decompress_block(stream, at, out_len)
        p = sc.judge(job, st, out)
        if p:
            problems.append(p)
        accepted += st == 0
        rejected += st != 0
print("accepted", accepted, "rejected", rejected)
for p in problems:
    print("PROBLEM", p)
print("ok" if not problems else "failed")
"""


def _run(kind):
    out = subprocess.run([sys.executable, "-c", _CHILD, HERE, kind], capture_output=True, text=True, timeout=1500)
    lines = out.stdout.strip().splitlines()
    last_job = next((ln for ln in reversed(lines) if ln.startswith("job ")), "none")
    problems = [ln for ln in lines if ln.startswith("PROBLEM")]
    assert out.returncode == 0, ("the emulator ended with status %d (negative: a signal, i.e. an access outside a guarded buffer) on %s"
                                 % (out.returncode, last_job), out.stderr[-1500:])
    assert lines and lines[-1] == "ok", (problems[:10], lines[-3:])
    counts = next(ln for ln in reversed(lines) if ln.startswith("accepted ")).split()
    return int(counts[1]), int(counts[3])


def test_the_model_of_the_interior_windows():
    """steady_end as the cases assume it: no steady window below 200 bytes when the block ends the stream, exactly one from 200
    to 263, and 200 bytes behind the block make every full window but none of a partial one interior."""
    import k2_steady_cases as sc
    assert [sc.steady_end(c, c) for c in (63, 199, 200, 263, 264, 327, 328)] == [0, 0, 64, 64, 128, 128, 192]
    assert [sc.steady_end(c, c + 200) for c in (63, 64, 127, 128, 199, 360)] == [0, 64, 64, 128, 192, 320]
    assert [sc.steady_end(c, c + 72) for c in (127, 128, 191, 192, 255, 256)] == [0, 64, 64, 128, 128, 192]
    assert sc.steady_end(sc.DEFECT_CSZ, sc.DEFECT_CSZ) == 192 and len(sc.hand_jobs()) == len({j[0] for j in sc.hand_jobs()})


def test_hand_made_blocks_at_the_seams_of_the_two_loops():
    accepted, rejected = _run("hand")
    assert accepted >= 1500 and rejected == 30           # the 15 defects, with 0 and 200 bytes behind the block


def test_every_block_of_intact_element_streams_decoded_alone():
    """Flavours 0-3 x block sizes 64, 700, 4097, 32768, the last block partial: every block accepted, bytes equal."""
    accepted, rejected = _run("intact")
    assert accepted >= 48 and rejected == 0


def test_the_same_bodies_as_raw_streams():
    """k2_decode_block<true>: the size word stripped, the header of the output length in front."""
    accepted, rejected = _run("raw")
    assert accepted >= 60 and rejected == 15
