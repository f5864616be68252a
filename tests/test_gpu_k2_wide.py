"""GPU (-m gpu): the wide block decoder (snappy_hip_decompress_blocks_wide, a workgroup per block) held to K2 on the same
device and to the oracle.  Every job of tests/k2_window_cases.py and of tests/k2_wide_cases.py is a call of its own --
total_len = block_size = that block's output length, a one-entry offset array -- into ONE arena filled with ranges_cases.GUARD,
ranges_cases.GAP guard bytes between the windows; the same jobs go through snappy_hip_decompress_blocks_batch into a second
arena.  Status and bytes must be K2's, the result words follow from K2's status and the limits alone
(k2_wide_cases.expected_result), and every guard byte is still there.  The wide call's own output is never a yardstick.  The
generated blocks, trips and small containers of k2_wide_cases are held to its model as well (verdict, bytes, result words),
each block at all four workgroup sizes.  These
inputs are rejected by bounds checks; none is built to fault."""
import hashlib
import os

import numpy as np
import pytest

import k2_wide_cases as wc
import k2_window_cases as kc
import ranges_cases as rcases
from conftest import GOLDEN, XML_TXT_LEN, XML_TXT_SHA256, golden_bytes

pytestmark = pytest.mark.gpu

ALL_WAVES = (2, 4, 8, 16)
JUNK = 0x5A5A5A5A


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


def _both_decoders(shb, jobs, shift=0):
    """every job through K2 (one batch call) and through the wide call (one call each, W by turns, `shift` turns on) ->
    (K2 statuses, K2 arena, wide statuses, wide arena, result words per job, destination offsets)"""
    import torch
    streams = sorted({j[1] for j in jobs}, key=len)
    index = {s: k for k, s in enumerate(streams)}
    d_streams, soffs = _stream_arena(streams)
    dst, arena_len = rcases.layout([j[3] for j in jobs])
    d_k2 = torch.full((arena_len,), rcases.GUARD, dtype=torch.uint8, device="cuda")
    d_wide = torch.full((arena_len,), rcases.GUARD, dtype=torch.uint8, device="cuda")
    d_k2_status = torch.full((len(jobs),), 7, dtype=torch.int32, device="cuda")
    d_wide_status = torch.full((len(jobs) + 1,), 7, dtype=torch.int32, device="cuda")
    d_result = torch.full((len(jobs) + 1, 4), 7, dtype=torch.int32, device="cuda")
    d_offs = torch.from_numpy(np.array([j[2] for j in jobs], dtype=np.int64)).cuda()
    batch = []
    for k, (name, stream, at, out_len) in enumerate(jobs):
        so = soffs[index[stream]]
        batch.append((d_streams[so:], len(stream), d_offs[k:k + 1], out_len, d_k2[dst[k]:], d_k2_status[k:k + 1]))
        shb.decompress_blocks_wide(d_streams[so:], len(stream), d_offs[k:k + 1], out_len, out_len, d_wide[dst[k]:], d_wide_status[k:k + 1],
                                   d_result[k], ALL_WAVES[(k + shift) % 4])
    shb.decompress_blocks_batch(batch, 65535)
    torch.cuda.synchronize()
    assert int(d_wide_status[len(jobs)]) == 7 and (d_result[len(jobs)].cpu().numpy() == 7).all()      # nothing behind the arrays
    return (d_k2_status.cpu().numpy(), d_k2.cpu().numpy(), d_wide_status.cpu().numpy()[:len(jobs)], d_wide.cpu().numpy(),
            d_result.cpu().numpy()[:len(jobs)], dst)


def _check(jobs, answers, shift=0):
    k2_status, k2_arena, status, arena, results, dst = answers
    problems, accepted, wide_path, expected = [], 0, 0, []
    for k, job in enumerate(jobs):
        name, stream, at, out_len = job
        st, k2_st = int(status[k]), int(k2_status[k])
        out = arena[dst[k]:dst[k] + out_len].tobytes()
        p = kc.check_job(job, st, out)                                    # the oracle
        if p is None and st != k2_st:
            p = "%s: status %d, K2's is %d" % (name, st, k2_st)
        if p is None and st == 0 and out != k2_arena[dst[k]:dst[k] + out_len].tobytes():
            p = name + ": bytes differ from K2's"
        if p is None and st != 0 and wc.must_accept(job):
            p = name + ": a valid block was rejected"
        want = wc.expected_result([(wc.within(stream, at, out_len), k2_st)])
        if p is None and [int(x) for x in results[k]] != want:
            p = "%s: result words %r, expected %r" % (name, [int(x) for x in results[k]], want)
        if p:
            problems.append("W=%d %s" % (ALL_WAVES[(k + shift) % 4], p))
        accepted += st == 0
        wide_path += int(results[k][0])
        expected.append((dst[k], out_len, "any"))                         # inside its window a rejected block may hold anything
    problems += rcases.check_buffer(arena, expected)                      # ... outside the windows: zero overwritten guard bytes
    return problems, accepted, wide_path


def test_intact_blocks_take_the_wide_path(shb):
    jobs = kc.intact_jobs()
    problems, accepted, wide_path = _check(jobs, _both_decoders(shb, jobs))
    assert not problems, problems[:10]
    assert accepted == len(jobs) and wide_path == sum(1 for j in jobs if j[3] <= wc.WIDE_MAX_BLOCK)


def test_hand_made_and_damaged_blocks_get_k2s_answers_and_leave_every_guard_byte(shb):
    jobs = kc.hand_jobs() + kc.damaged_jobs(300)
    problems, accepted, wide_path = _check(jobs, _both_decoders(shb, jobs))
    assert not problems, (len(problems), problems[:10])
    assert 0 < wide_path <= accepted < len(jobs)


def test_hand_built_blocks_aimed_at_the_wide_path(shb, monkeypatch):
    jobs = wc.hand_jobs()
    for cap in (None, "3"):                                               # the default grid, and three workgroups at most
        if cap:
            monkeypatch.setenv("SNAPPY_HIP_K2_WAVES", cap)
        # twice over, the second time shifted by one: every job meets two workgroup sizes
        for shift in (0, 1):
            turn = jobs[shift:] + jobs[:shift]
            problems, accepted, wide_path = _check(turn, _both_decoders(shb, turn))
            assert not problems, (cap, problems[:10])
            assert 0 < wide_path < len(jobs)


@pytest.fixture(scope="module")
def generated():
    """the generated blocks of k2_wide_cases as jobs, made once"""
    return wc.block_jobs(wc.small_blocks() + wc.large_blocks())


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_generated_blocks_against_k2_the_oracle_and_the_model(shb, generated, shift):
    """k2_wide_cases.small_blocks and large_blocks (tests/test_k2_wide_model.py holds them to their coverage conditions), every
    block at all four workgroup sizes over the four turns: K2's and the oracle's status and bytes (_check), and the model's
    verdict, bytes and result words.  The invalid ones are rejected by bounds checks; none is built to fault."""
    answers = _both_decoders(shb, generated, shift)
    problems, accepted, wide_path = _check(generated, answers, shift)
    status, arena, results, dst = answers[2], answers[3], answers[4], answers[5]
    valid = 0
    for k, job in enumerate(generated):
        waves = ALL_WAVES[(k + shift) % 4]
        m = wc.job_model(job, waves)
        valid += m.valid
        if int(status[k]) != (0 if m.valid else 1):
            problems.append("W=%d %s: status %d, the model says valid = %r" % (waves, job[0], int(status[k]), m.valid))
        elif m.valid and arena[dst[k]:dst[k] + job[3]].tobytes() != m.out:
            problems.append("W=%d %s: bytes differ from the model's" % (waves, job[0]))
        elif [int(x) for x in results[k]] != m.words:
            problems.append("W=%d %s: result words %r, the model's %r" % (waves, job[0], [int(x) for x in results[k]], m.words))
    assert not problems, (len(problems), problems[:10])
    assert accepted == valid and wide_path == valid - 1                   # (one valid block lies beyond the csz limit)


def _whole(shb, stream, offs, total, bs, waves):
    """one container through K2 and through the wide call, its output behind GAP guard bytes ->
    (K2 statuses, K2 bytes, wide statuses, wide bytes, result words); every guard byte and every word behind the arrays tested"""
    import torch
    d_stream, _ = _stream_arena([stream])
    d_offs = torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()
    d_k2_out = torch.full((total,), rcases.GUARD, dtype=torch.uint8, device="cuda")
    d_k2_status = torch.full((len(offs),), 7, dtype=torch.int32, device="cuda")
    shb.decompress_blocks(d_stream, len(stream), d_offs, total, bs, d_k2_out, d_k2_status)
    d_out = torch.full((rcases.GAP + total + 64,), rcases.GUARD, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(offs) + 1,), 7, dtype=torch.int32, device="cuda")
    d_result = torch.full((5,), 7, dtype=torch.int32, device="cuda")
    shb.decompress_blocks_wide(d_stream, len(stream), d_offs, total, bs, d_out[rcases.GAP:], d_status, d_result, waves)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:rcases.GAP] == rcases.GUARD).all() and (out[rcases.GAP + total:] == rcases.GUARD).all(), waves
    status, result = [int(x) for x in d_status.cpu().numpy()], [int(x) for x in d_result.cpu().numpy()]
    assert status[len(offs)] == 7 and result[4] == 7, waves
    return ([int(x) for x in d_k2_status.cpu().numpy()], d_k2_out.cpu().numpy().tobytes(), status[:len(offs)],
            out[rcases.GAP:rcases.GAP + total].tobytes(), result[:4])


def test_trips_one_workgroup_meets_every_block_of_a_container_in_turn(shb, monkeypatch):
    """k2_wide_cases.trips as whole-container calls with SNAPPY_HIP_K2_WAVES=1, which caps the wide call's grid at ONE workgroup:
    what a trip leaves in LDS meets the next block.  Statuses, bytes and the summed result words are the model's and K2's."""
    monkeypatch.setenv("SNAPPY_HIP_K2_WAVES", "1")
    for name, stream, offs, total, bs, blocks in wc.trips():
        for waves in ALL_WAVES:
            models = [wc.model(body, n, waves) for body, n in blocks]
            k2_status, k2_out, status, out, result = _whole(shb, stream, offs, total, bs, waves)
            assert status == k2_status == [0 if m.valid else 1 for m in models], (name, waves, status)
            assert result == [sum(m.words[i] for m in models) for i in range(4)], (name, waves, result)
            for b, m in enumerate(models):
                if m.valid:
                    assert out[b * bs:b * bs + m.out_len] == m.out == k2_out[b * bs:b * bs + m.out_len], (name, waves, b)


@pytest.mark.parametrize("cap", [None, "1"])
def test_small_block_sizes_every_alignment_of_a_window(shb, monkeypatch, cap):
    """100 blocks of 17 bytes -- with step F's head, middle and tail every alignment of a window against out_len 17 -- and block
    sizes 1, 15, 16, 31, 33 and 48, behind GAP guard bytes, at all four workgroup sizes: the plaintext, K2's bytes, [0] = the
    block count"""
    if cap:
        monkeypatch.setenv("SNAPPY_HIP_K2_WAVES", cap)
    for name, stream, plain, offs, total, bs in wc.small_containers():
        for waves in ALL_WAVES:
            k2_status, k2_out, status, out, result = _whole(shb, stream, offs, total, bs, waves)
            assert status == k2_status == [0] * len(offs), (name, waves)
            assert out == plain == k2_out, (name, waves)
            assert result == [len(offs), 0, 0, 0], (name, waves)


def _golden_plain_ok(name, out):
    if name == "xml":
        return len(out) == XML_TXT_LEN and hashlib.sha256(out).hexdigest() == XML_TXT_SHA256
    return out == golden_bytes(name + ".txt")


@pytest.mark.parametrize("cap", [None, "3"])
def test_goldens_whole_at_every_workgroup_size(shb, monkeypatch, cap):
    import torch
    if cap:
        monkeypatch.setenv("SNAPPY_HIP_K2_WAVES", cap)
    for name in ("terror2", "alice", "coding", "plrabn12", "xml"):
        stream = golden_bytes(name + ".snappy")
        total, bs, offs = kc._offsets(stream)
        d_stream, _ = _stream_arena([stream])
        d_offs = torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()
        d_k2_out = torch.full((total,), rcases.GUARD, dtype=torch.uint8, device="cuda")
        d_k2_status = torch.full((len(offs),), 7, dtype=torch.int32, device="cuda")
        shb.decompress_blocks(d_stream, len(stream), d_offs, total, bs, d_k2_out, d_k2_status)
        for waves in ALL_WAVES if cap is None else (16,):
            d_out = torch.full((total + 64,), rcases.GUARD, dtype=torch.uint8, device="cuda")
            d_status = torch.full((len(offs) + 1,), 7, dtype=torch.int32, device="cuda")
            d_result = torch.full((5,), 7, dtype=torch.int32, device="cuda")
            shb.decompress_blocks_wide(d_stream, len(stream), d_offs, total, bs, d_out, d_status, d_result, waves)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            assert _golden_plain_ok(name, out[:total].tobytes()), (name, waves)
            assert torch.equal(d_out[:total], d_k2_out) and (out[total:] == rcases.GUARD).all(), (name, waves)
            assert torch.equal(d_status[:len(offs)], d_k2_status) and (d_status.cpu().numpy()[:len(offs)] == 0).all(), (name, waves)
            assert [int(x) for x in d_result.cpu().numpy()] == [len(offs), 0, 0, 0, 7] and int(d_status[len(offs)]) == 7, (name, waves)


def test_a_block_size_above_the_limit_goes_serial_and_a_damaged_container_gets_k2s_statuses(shb):
    import torch
    name, stream, plain, offs, total, bs = wc.serial_container()
    terror = golden_bytes("terror2.snappy")
    t_total, t_bs, t_offs = kc._offsets(terror)
    bad = bytearray(terror)
    bad[t_offs[1] + 4] = bad[t_offs[3] + 4] = 0xFF
    for s, o, tot, b, want_res, want_st in ((stream, offs, total, bs, [0, len(offs), 0, 0], [0] * len(offs)),
                                            (bytes(bad), t_offs, t_total, t_bs, [2, 0, 2, 0], [0, 1, 0, 1])):
        d_stream, _ = _stream_arena([s])
        d_offs = torch.from_numpy(np.array(o, dtype=np.int64)).cuda()
        d_out = torch.full((tot,), rcases.GUARD, dtype=torch.uint8, device="cuda")
        d_status = torch.full((len(o),), 7, dtype=torch.int32, device="cuda")
        d_k2_out, d_k2_status = d_out.clone(), d_status.clone()
        d_result = torch.full((4,), 7, dtype=torch.int32, device="cuda")
        shb.decompress_blocks(d_stream, len(s), d_offs, tot, b, d_k2_out, d_k2_status)
        shb.decompress_blocks_wide(d_stream, len(s), d_offs, tot, b, d_out, d_status, d_result)
        torch.cuda.synchronize()
        assert [int(x) for x in d_status.cpu().numpy()] == [int(x) for x in d_k2_status.cpu().numpy()] == want_st
        assert [int(x) for x in d_result.cpu().numpy()] == want_res
        for k, st in enumerate(want_st):
            if st == 0:
                assert torch.equal(d_out[k * b:(k + 1) * b], d_k2_out[k * b:(k + 1) * b])
    assert bytes(d_k2_out[:t_bs].cpu().numpy()) == golden_bytes("terror2.txt")[:t_bs]


def test_arguments(shb):
    import torch
    stream = golden_bytes("coding.snappy")
    total, bs, offs = kc._offsets(stream)
    d_stream, _ = _stream_arena([stream])
    d_offs = torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()
    d_out = torch.full((total,), rcases.GUARD, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(offs),), 7, dtype=torch.int32, device="cuda")
    d_result = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    lib = shb.lib()
    good = [d_stream.data_ptr(), len(stream), d_offs.data_ptr(), total, bs, d_out.data_ptr(), d_status.data_ptr(), 0, d_result.data_ptr(), None]
    for k, v in ((0, None), (2, None), (5, None), (6, None), (8, None), (4, 0), (4, 65536), (7, 1), (7, 3), (7, 32), (7, 64)):
        bad = list(good)
        bad[k] = v
        assert lib.snappy_hip_decompress_blocks_wide(*bad) == 2, (k, v)                       # SNAPPY_HIP_ERR_ARG
    no_result = list(good)
    no_result[3], no_result[8] = 0, None
    assert lib.snappy_hip_decompress_blocks_wide(*no_result) == 2
    torch.cuda.synchronize()                                                                   # a refused call enqueues nothing
    assert (d_result.cpu().numpy() == 7).all() and (d_status.cpu().numpy() == 7).all() and (d_out.cpu().numpy() == rcases.GUARD).all()
    empty = list(good)
    empty[3] = 0                                                                               # total_len == 0: nothing launched, d_result = 0
    assert lib.snappy_hip_decompress_blocks_wide(*empty) == 0
    torch.cuda.synchronize()
    assert (d_result.cpu().numpy() == 0).all() and (d_status.cpu().numpy() == 7).all() and (d_out.cpu().numpy() == rcases.GUARD).all()
    d_result.fill_(7)
    assert lib.snappy_hip_decompress_blocks_wide(*good) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in d_result.cpu().numpy()] == [len(offs), 0, 0, 0]
    assert bytes(d_out.cpu().numpy()) == golden_bytes("coding.txt")


def test_the_drop_in_call_and_the_cli(shb, tmp_path):
    import subprocess
    from test_cli import CLI, HOST_DIR, check_stdout_contract, run
    subprocess.check_call(["make", "-s", "-C", HOST_DIR])
    plain = golden_bytes("terror2.txt")
    stream = golden_bytes("terror2.snappy")
    for waves in (0, 4):
        st, out, rt = shb.decompress_host_wide(stream, waves)
        assert st == shb.SNAPPY_OK and out == plain and rt["run"] > 0
    assert shb.decompress_host(stream)[:2] == (shb.SNAPPY_OK, plain)                           # the same file, the same statuses
    assert shb.decompress_host_wide(stream, 3)[0] == shb.SNAPPY_INVALID_INPUT
    _, _, offs = kc._offsets(stream)
    bad = bytearray(stream)
    bad[offs[2] + 4] = 0xFF
    assert shb.decompress_host_wide(bytes(bad))[0] == shb.SNAPPY_INVALID_INPUT == shb.decompress_host(bytes(bad))[0]
    assert shb.decompress_host_wide(stream[:-1])[0] == shb.SNAPPY_INVALID_INPUT
    assert shb.decompress_host_wide(stream, 0, len(plain) - 1)[0] == shb.SNAPPY_BUFFER_TOO_SMALL
    st, out, _ = shb.decompress_host_wide(stream, 0, len(plain))
    assert st == shb.SNAPPY_OK and out == plain
    src = os.path.join(GOLDEN, "plrabn12.txt")
    packed = tmp_path / "p.snappy"
    r = run(CLI, "-d", "-c", "-b", "32768", "-i", src, "-o", str(packed))
    assert r.returncode == 0, r.stderr
    for flag in ("-W", "-W4"):
        back = tmp_path / ("back" + flag)
        r = run(CLI, "-d", flag, "-i", str(packed), "-o", str(back))
        assert r.returncode == 0, (flag, r.stderr)
        check_stdout_contract(r.stdout)
        assert back.read_bytes() == golden_bytes("plrabn12.txt"), flag
