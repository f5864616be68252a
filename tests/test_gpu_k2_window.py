"""GPU (-m gpu): K2 writes only inside a block's output window.  The blocks of tests/k2_window_cases.py -- every block of
intact element streams, the damaged blocks of 300 damaged streams, hand-made blocks aimed at the output bound -- go through
snappy_hip_decompress_blocks_batch with every block a job of its own: total_len = that block's output length, a one-entry
offset array, and d_out pointing into ONE arena filled with ranges_cases.GUARD, ranges_cases.GAP guard bytes between the
windows (GAP is odd: the windows meet every alignment).  Afterwards every byte that no window owns is still GUARD.  The
emulator runs the same jobs between inaccessible pages (tests/test_k2_window_emulated.py); these inputs are rejected by a
bounds check, none is built to fault."""
import numpy as np
import pytest

import k2_window_cases as kc
import ranges_cases as rcases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return binding


def _stream_arena(streams):
    """All streams in one device buffer, 16 bytes of padding behind each -> (tensor, offsets)."""
    import torch
    offs, at = [], 0
    for s in streams:
        offs.append(at)
        at += (len(s) + 16 + 15) & ~15
    host = np.zeros(at + 16, dtype=np.uint8)
    for s, o in zip(streams, offs):
        host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), offs


def _decode_each_block_alone(shb, jobs):
    """-> (statuses, arena bytes, destination offsets) after one batch call over all jobs."""
    import torch
    streams = sorted({j[1] for j in jobs}, key=len)
    index = {s: k for k, s in enumerate(streams)}
    d_streams, soffs = _stream_arena(streams)
    dst, arena_len = rcases.layout([j[3] for j in jobs])
    d_arena = torch.full((arena_len,), rcases.GUARD, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(jobs),), 7, dtype=torch.int32, device="cuda")
    d_offs = torch.from_numpy(np.array([j[2] for j in jobs], dtype=np.int64)).cuda()
    batch = []
    for k, (name, stream, at, out_len) in enumerate(jobs):
        so = soffs[index[stream]]
        batch.append((d_streams[so:], len(stream), d_offs[k:k + 1], out_len, d_arena[dst[k]:], d_status[k:k + 1]))
    # one call; with the largest block size every job is a one-block container of exactly its total_len bytes
    shb.decompress_blocks_batch(batch, 65535)
    torch.cuda.synchronize()
    return d_status.cpu().numpy(), d_arena.cpu().numpy(), dst


def _check(jobs, status, arena, dst):
    expected, problems, accepted = [], [], 0
    for k, job in enumerate(jobs):
        out_len = job[3]
        st = int(status[k])
        out = arena[dst[k]:dst[k] + out_len].tobytes()
        p = kc.check_job(job, st, out)
        if p is None and st != 0 and kc.must_accept(job):
            p = job[0] + ": a valid block was rejected"
        if p:
            problems.append(p)
        accepted += st == 0
        expected.append((dst[k], out_len, "any"))            # inside its window a rejected block may hold anything
    problems += rcases.check_buffer(arena, expected)          # ... outside the windows: zero overwritten guard bytes
    return problems, accepted


def test_intact_blocks_each_in_its_own_guarded_window(shb):
    jobs = kc.intact_jobs()
    status, arena, dst = _decode_each_block_alone(shb, jobs)
    problems, accepted = _check(jobs, status, arena, dst)
    assert not problems, problems[:10]
    assert accepted == len(jobs)


def test_hand_made_and_damaged_blocks_leave_every_guard_byte(shb):
    jobs = kc.hand_jobs() + kc.damaged_jobs(300)
    status, arena, dst = _decode_each_block_alone(shb, jobs)
    problems, accepted = _check(jobs, status, arena, dst)
    assert not problems, (len(problems), problems[:10])
    assert 0 < accepted < len(jobs)                          # neither everything rejected nor everything accepted


def test_whole_containers_into_exactly_total_len_bytes(shb):
    """snappy_hip_decompress_blocks with an output of exactly total_len bytes inside a guarded arena."""
    import torch
    import oracle_lib as oracle
    conts = kc.intact_containers()
    dst, arena_len = rcases.layout([len(p) for _, _, p in conts])
    d_arena = torch.full((arena_len,), rcases.GUARD, dtype=torch.uint8, device="cuda")
    keep = []
    for k, (name, stream, plain) in enumerate(conts):
        total, bs, _ = oracle.read_header(stream)
        offs = oracle.index_blocks(stream).astype(np.int64)
        d_stream, _ = _stream_arena([stream])
        d_offs = torch.from_numpy(offs).cuda()
        d_status = torch.full((len(offs),), 7, dtype=torch.int32, device="cuda")
        shb.decompress_blocks(d_stream, len(stream), d_offs, total, bs, d_arena[dst[k]:], d_status)
        keep.append((d_stream, d_offs, d_status))
    torch.cuda.synchronize()
    for name, (_, _, d_status) in zip((c[0] for c in conts), keep):
        assert (d_status.cpu().numpy() == 0).all(), name
    problems = rcases.check_buffer(d_arena.cpu().numpy(), [(dst[k], len(p), p) for k, (_, _, p) in enumerate(conts)])
    assert not problems, problems[:10]
