"""GPU (-m gpu): the two window loops of k2_decode_block (csrc/snappy_kernels.hpp).  The blocks of tests/k2_steady_cases.py --
compressed sizes around the first interior windows at every alignment and with 0 to 200 bytes of stream behind the block,
literals that run on out of a steady window, defects in the first, a middle and the last steady window, every block of the
intact element streams -- go through snappy_hip_decompress_blocks_batch with every block a job of its own, its output window
between guard bytes (the arena of tests/test_gpu_k2_window.py), and as raw streams through snappy_hip_raw_decompress_batch
(the arena of tests/test_gpu_raw.py).  The emulator runs the same jobs between inaccessible pages
(tests/test_k2_steady_emulated.py); the defects are rejected by a bounds check, none is built to fault."""
import pytest

import k2_steady_cases as sc
import ranges_cases as rcases
import raw_cases as rc
import test_gpu_k2_window as window
import test_gpu_raw as raw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return binding


def _decode_and_judge(shb, jobs):
    status, arena, dst = window._decode_each_block_alone(shb, jobs)
    problems, accepted, expected = [], 0, []
    for k, job in enumerate(jobs):
        st = int(status[k])
        p = sc.judge(job, st, arena[dst[k]:dst[k] + job[3]].tobytes())
        if p:
            problems.append(p)
        accepted += st == 0
        expected.append((dst[k], job[3], "any"))             # inside its window a rejected block may hold anything
    problems += rcases.check_buffer(arena, expected)          # ... outside the windows: zero overwritten guard bytes
    return problems, accepted


def test_hand_made_blocks_at_the_seams_of_the_two_loops(shb):
    jobs = sc.hand_jobs()
    problems, accepted = _decode_and_judge(shb, jobs)
    assert not problems, (len(problems), problems[:10])
    assert len(jobs) - accepted == 30                         # the 15 defects, with 0 and 200 bytes behind the block


def test_intact_blocks_each_in_its_own_guarded_window(shb):
    jobs = sc.intact_jobs()
    problems, accepted = _decode_and_judge(shb, jobs)
    assert not problems, problems[:10]
    assert accepted == len(jobs) >= 48


def test_the_same_bodies_as_raw_streams(shb):
    """k2_decode_block<true> in one launch; raw.Batch.fetch() checks the guard bytes between the windows."""
    items = sc.raw_items()
    b = raw.gpu_decompress(shb, [(s, n) for _, s, n in items])
    problems = [p for p in (sc.judge_raw(item, b.status[i], b.out_len[i], b.window(i)) for i, item in enumerate(items)) if p]
    assert not problems, problems[:10]
    assert b.status[:b.n].count(rc.INVALID) == 15 and b.status[:b.n].count(rc.OK) == b.n - 15
