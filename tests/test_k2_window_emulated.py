"""K2 writes only inside a block's output window (k2_decode_block: "nothing outside it written whatever the stream
holds"), on the CPU wave emulator: every block of tests/k2_window_cases.py is decoded ALONE into a buffer of exactly its
output length that ends at an inaccessible page and starts behind one, its stream in front of an inaccessible page too.
One byte written behind the window, or read behind the stream, is a fault -- a legitimate failure here, so the decoding
runs in a child process that names the job it is on before it starts it."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import emu_lib as emu, k2_window_cases as kc
jobs = {"intact": kc.intact_jobs, "hand": kc.hand_jobs, "damaged": lambda: kc.damaged_jobs(int(sys.argv[3]))}[sys.argv[2]]()
problems, accepted = [], 0
for job in jobs:
    name, stream, at, out_len = job
    print("job", name, flush=True)
    st, out = emu.decompress_block(stream, at, out_len)
    p = kc.check_job(job, st, out)
    if p is None and st != 0 and kc.must_accept(job):
        p = name + ": a valid block was rejected"
    if p:
        problems.append(p)
    accepted += st == 0
print("jobs", len(jobs), "accepted", accepted)
for p in problems:
    print("PROBLEM", p)
print("ok" if not problems and accepted > 0 else "failed")
"""


def _run(kind, count=0):
    out = subprocess.run([sys.executable, "-c", _CHILD, HERE, kind, str(count)], capture_output=True, text=True, timeout=1500)
    lines = out.stdout.strip().splitlines()
    last_job = next((ln for ln in reversed(lines) if ln.startswith("job ")), "none")
    problems = [ln for ln in lines if ln.startswith("PROBLEM")]
    assert out.returncode == 0, ("the emulator ended with status %d (negative: a signal, i.e. an access outside a guarded buffer) on %s"
                                 % (out.returncode, last_job), out.stderr[-1500:])
    assert lines and lines[-1] == "ok", (problems[:10], lines[-3:])
    return lines


def test_every_block_of_intact_element_streams_decoded_alone():
    """Flavours 0-3 x block sizes 64, 700, 4097, 32768, 65535, last block partial: every block accepted, bytes equal."""
    lines = _run("intact")
    jobs, accepted = (int(x) for x in lines[-2].split()[1::2])
    assert jobs == accepted and jobs >= 60


def test_hand_made_blocks_at_the_output_bound():
    """Literals with 4-byte lengths of 0xffffffff, 0xfffffffe, out_len - op + {0, 1, 2^32 - 64}; windows whose element
    lengths sum past 2^32 and 2^16; copies and spilling literals that end at and one past out_len; out_len 1, 63, 64, 65 and
    65535.  The expected status is the oracle's (K2 may be stricter, never laxer); blocks that are valid must be accepted."""
    _run("hand")


def test_damaged_blocks_decoded_alone():
    """300 damaged element streams (the recipe of the damaged-stream tests), every block that holds a damaged byte."""
    _run("damaged", 300)


def test_whole_containers_unpadded():
    """emu_lib.decompress gives K2 exactly total_len bytes between inaccessible pages: the intact containers as a whole."""
    import emu_lib as emu
    import k2_window_cases as kc
    import oracle_lib as oracle
    child = ("import sys; sys.path.insert(0, sys.argv[1]); import emu_lib as emu, k2_window_cases as kc, oracle_lib as oracle\n"
             "for name, stream, plain in kc.intact_containers():\n"
             "    total, bs, hdr = oracle.read_header(stream)\n"
             "    print('job', name, flush=True)\n"
             "    st, out = emu.decompress(stream, total, bs, hdr)\n"
             "    assert st == 0 and out == plain, name\n"
             "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", child, HERE], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-300:], out.stderr[-1500:])
