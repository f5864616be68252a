"""The wide block decoder's cases judged by the model alone (tests/k2_wide_cases.py: model, generators).  No
emulator, no GPU, and no word of the kernel's output: every condition below is computed from one serial Python walk of the
blocks, so the inputs of tests/test_k2_wide_emulated.py and tests/test_gpu_k2_wide.py cannot quietly stop covering a share
boundary, a window position or a copy chain.  The model's verdict and bytes are held to the oracle here."""
import functools

import pytest

import k2_wide_cases as wc
import k2_window_cases as kc

KINDS = {"literal1": 1, "literal2": 2, "literal3": 3, "literal4": 4, "literal5": 5, "copy1": 2, "copy2": 3, "copy4": 5}   # kind: header bytes


@functools.lru_cache(maxsize=None)
def _blocks():
    return tuple(wc.small_blocks() + wc.large_blocks())


@functools.lru_cache(maxsize=None)
def _models(waves):
    """(block, model at `waves`) of every generated block aimed at that workgroup size or at any"""
    return tuple((b, wc.model(b[1], b[2], waves)) for b in _blocks() if b[3] in (None, waves))


def _which(s, last):
    return "first" if s == 1 else ("last" if s == last else "middle")


def test_names_and_verdicts_agree_and_valid_blocks_are_expected_on_the_wide_path():
    names = [b[0] for b in _blocks()]
    assert len(set(names)) == len(names)
    for waves in wc.ALL_WAVES:
        for (name, body, out_len, _), m in _models(waves):
            assert m.valid == name.startswith("valid"), (waves, name)
            want = wc.BEYOND if len(body) > wc.WIDE_MAX_CSZ else (wc.WIDE if m.valid else wc.UNPROVEN)
            assert m.words == want, (waves, name)
            assert m.words == wc.expected_result([(wc.within(wc.block_jobs([(name, body, out_len, None)])[0][1], len(kc._varint(out_len)) * 2, out_len),
                                                   0 if m.valid else 1)]), name
    sizes = {b[0]: (len(b[1]), b[2]) for b in wc.large_blocks()}
    assert len(sizes) <= 10 and all(b[2] <= wc.WIDE_MAX_BLOCK for b in _blocks())


def test_the_models_verdict_and_bytes_are_the_oracles():
    """on every generated block, but that the model has K2's stricter verdict where the oracle stops at out_len and lets an
    element run past it; on the older jobs within the limits the model may be K2's stricter self too
    (k2_window_cases.check_job allows that direction only), never more lenient"""
    for job in wc.block_jobs(_blocks()):
        m = wc.job_model(job, 2)
        st, out = kc.expect(job[1], job[2], job[3])
        if st == 0 and not m.valid:
            assert "past out_len" in job[0] or "passes out_len" in job[0], job[0]
        else:
            assert (0 if m.valid else 1) == st and m.out == out, job[0]
    for job in kc.intact_jobs() + wc.hand_jobs() + kc.hand_jobs():
        if not wc.within(job[1], job[2], job[3]):
            continue
        m = wc.job_model(job, 16)
        st, out = kc.expect(job[1], job[2], job[3])
        if m.valid:
            assert st == 0 and m.out == out, job[0]
        else:
            assert not wc.must_accept(job), job[0]


@pytest.mark.parametrize("waves", wc.ALL_WAVES)
def test_every_element_kind_meets_every_share_boundary_at_every_distance(waves):
    """first, middle and last boundary x kind x tag d = 0 .. header bytes in front of the boundary"""
    seen = set()
    for _, m in _models(waves):
        if not m.valid:
            continue
        last = (m.csz - 1) // m.share
        for e in m.elements:
            for s in range(max(1, e.pos // m.share), last + 1):
                d = s * m.share - e.pos
                if 0 <= d <= e.hdr:
                    seen.add((_which(s, last), e.kind, d))
    whiches = {"first"} | ({"middle", "last"} if waves >= 4 else set())     # (two shares have one boundary)
    missing = [(w, k, d) for w in whiches for k, hdr in KINDS.items() for d in range(hdr + 1) if (w, k, d) not in seen]
    assert not missing, missing


@pytest.mark.parametrize("waves", wc.ALL_WAVES)
def test_the_chain_enters_shares_at_every_offset_from_the_table_and_by_walking(waves):
    """offsets 0-4 and 61-63 from the table, 64, 65 and 127 (128, 129 where a share holds them) walked by step C; behind every
    literal header length that a boundary splits"""
    seen, split_headers = set(), set()
    for _, m in _models(waves):
        if not m.valid:
            continue
        for s, sh in enumerate(m.shares):
            if sh is None or s == 0:
                continue
            assert sh["table"] == (sh["offset"] < 64)
            seen.add((sh["offset"], sh["table"]))
            if sh["offset"]:
                before = m.elements[sh["first"] - 1]
                cut = s * m.share - before.pos
                if before.type == wc.LITERAL and 0 < cut < before.hdr:
                    split_headers.add((before.hdr, cut))
    offsets = [t for t in wc.ENTRY_OFFSETS if t < wc.sweep_share(waves)]
    assert (waves == 16) == (len(offsets) < len(wc.ENTRY_OFFSETS))
    assert not [t for t in offsets if (t, t < 64) not in seen], sorted(seen)
    assert not [(h, c) for h in (2, 3, 4, 5) for c in range(1, h) if (h, c) not in split_headers]


@pytest.mark.parametrize("waves", wc.ALL_WAVES)
def test_literals_pass_over_whole_shares(waves):
    """one share, two shares and every remaining share passed over (W >= 4), a literal from share 0 to csz (every W), and at
    W = 16 the entries 0 and 1 behind one share passed over"""
    runs, to_the_end, after_one = set(), set(), set()
    for _, m in _models(waves):
        if not m.valid or not m.passed:
            continue
        last = (m.csz - 1) // m.share
        p = m.passed
        first = p[0]
        length = next(k for k in range(len(p) + 1) if k == len(p) or p[k] != first + k)
        if first + length - 1 == last:
            to_the_end.add(first - 1)                                    # the share the literal starts in
        else:
            runs.add(length)
            if length == 1:
                after_one.add(m.shares[first + 1]["offset"])
    assert 0 in to_the_end
    if waves >= 4:
        assert {1, 2} <= runs and 1 in to_the_end
    if waves == 16:
        assert {0, 1} <= after_one


def _runon_wanted():
    """what the window sweep must hold, from the arithmetic of wide_share_walk's run-on alone: a literal of `length` bytes with
    `hdr` header bytes and its tag at `lane` leaves n = length bytes behind the window when its payload starts behind it
    (ps = lane + hdr > 64), lane + hdr + length - 64 otherwise"""
    want = set()
    for lane in range(56, 64):
        for hdr in (1, 2, 3, 4, 5):
            for n in wc.RUNON_N:
                ps = lane + hdr
                length = n if ps > 64 else n + 64 - ps
                if 1 <= length <= wc.LITERAL_CAP[hdr]:
                    want |= {(lane, hdr, n, ending) for ending in ("last", "literal", "copy")}
    return want


def test_the_window_sweep_holds_every_tag_lane_header_and_run_on_length():
    seen, copies = {}, set()
    for (name, _, _, _), m in _models(2):
        if not m.valid or " window " not in name:
            continue
        for w in m.windows:
            r = w["runon"]
            if r and w["share"] == 1:                                   # (inside one share: the last one)
                assert r["frm"] == max(r["ps"], 64) and r["n"] >= 1
                seen[(r["lane"], r["hdr"], r["n"], r["ending"])] = r
            e = w["elements"][-1]
            if e.type != wc.LITERAL:
                copies.add((e.pos - w["g"], e.kind))
    want = _runon_wanted()
    assert len(want) > 1000 and not want - set(seen), sorted(want - set(seen))[:10]
    rs = [seen[k] for k in want]
    assert {r["branch"] for r in rs} == {"n<4", "n>=4 mod 0", "n>=4 mod 1", "n>=4 mod 2", "n>=4 mod 3"}
    assert {r["passes"] for r in rs} == {1, 2}                          # n > 256: more than one pass of 64 lanes
    for hdr in (1, 2, 3, 4, 5):
        assert any(r["hdr"] == hdr and r["ps"] <= 64 for r in rs)
    for hdr in (2, 3, 4, 5):                                             # the payload starts behind the window
        for branch in ("n<4", "n>=4 mod 1"):
            assert any(r["hdr"] == hdr and r["ps"] > 64 and r["branch"] == branch for r in rs), (hdr, branch)
        assert any(r["hdr"] == hdr and r["ps"] > 64 and r["passes"] == 2 for r in rs) == (hdr > 2)
    assert not [(lane, k) for lane in range(59, 64) for k in ("copy1", "copy2", "copy4") if (lane, k) not in copies]


@pytest.mark.parametrize("waves", wc.ALL_WAVES)
def test_copy_chains_of_every_depth_and_across_the_shares(waves):
    rounds, pairs, firsts = set(), set(), set()
    cross_literal = cross_copy = False
    depth = 0
    for (name, _, _, _), m in _models(waves):
        last = (m.csz - 1) // m.share if m.csz else 0
        for s, sh in enumerate(m.shares):
            if sh and s and sh["offset"] == 0 and m.elements[sh["first"]].type != wc.LITERAL:
                e = m.elements[sh["first"]]
                how = "byte 0" if e.off == e.op else ("before" if e.off == e.op + 1 else ("zero" if e.off == 0 else None))
                if how and m.valid == (how == "byte 0"):
                    firsts.add((s, how))
        if not m.valid:
            continue
        if " chain of " in name:
            assert m.hops == m.out_len - 1 and not any(e.type == wc.LITERAL for e in m.elements[1:])
            rounds.add(m.rounds)
        pairs |= {(e.off, e.olen) for e in m.elements if e.type != wc.LITERAL}
        cross_literal |= m.cross_literal
        cross_copy |= m.cross_copy
        depth = max(depth, m.cross_depth)
    assert rounds == set(range(16))
    assert not [(o, n) for o in range(1, 9) for n in range(1, 65) if (o, n) not in pairs]
    assert cross_literal and cross_copy
    assert depth >= min(2, waves - 2)                                    # chained over three shares or more (two shares have one link)
    assert not [(s, h) for s in range(1, waves) for h in ("byte 0", "before", "zero") if (s, h) not in firsts]


@pytest.mark.parametrize("waves", wc.ALL_WAVES)
def test_the_output_bound_is_met_in_the_first_a_middle_and_the_last_share(waves):
    """the element that passes out_len does so by one byte, in the first, a middle and the last share (there it is the block's
    last: the output is one past out_len); an output one short of out_len; and a neighbour of each that fits exactly"""
    crossed, short, exact = set(), 0, 0
    for (name, _, _, _), m in _models(waves):
        total = sum(e.olen for e in m.elements)
        if "out_len" not in name or not m.elements:
            continue
        last = (m.csz - 1) // m.share
        over = next((e for e in m.elements if e.op + e.olen > m.out_len), None)
        if over is not None and over.op + over.olen == m.out_len + 1:
            s = over.pos // m.share
            crossed.add(("first" if s == 0 else ("last" if s == last else "middle"), over is m.elements[-1]))
            assert not m.valid and m.words == wc.UNPROVEN
        short += total == m.out_len - 1 and not m.valid
        exact += total == m.out_len and m.valid
    want = {("first", False), ("last", True)} | ({("middle", False)} if waves >= 4 else set())
    assert want <= crossed, crossed
    assert short >= len(want) and exact >= len(want)


def test_the_limits():
    by_name = {b[0]: b for b in wc.limit_blocks()}
    m = wc.model(*by_name["no compressed bytes at all"][1:3], 16)
    assert m.csz == 0 and not m.valid and m.words == wc.UNPROVEN
    m = wc.model(*by_name["valid csz at the limit"][1:3], 2)
    assert m.csz == wc.WIDE_MAX_CSZ == 38400 and len(m.elements) == 19200 and m.valid and m.words == wc.WIDE
    m = wc.model(*by_name["valid csz one past the limit"][1:3], 2)
    assert m.csz == wc.WIDE_MAX_CSZ + 1 and m.valid and m.words == wc.BEYOND
    m = wc.model(*by_name["valid run-on literal ends at out_len 32768"][1:3], 4)
    r = m.windows[-1]["runon"]
    assert m.valid and m.out_len == wc.WIDE_MAX_BLOCK and r["ending"] == "last" and r["passes"] > 1
    assert m.elements[-1].op + m.elements[-1].olen == wc.WIDE_MAX_BLOCK


def test_the_trips_meet_what_the_block_before_left_behind():
    """block sizes 700 and 4,097, at W = 2 and 16: a block that enters every share it has (several), then one whose chain passes
    over shares the first one entered -- their control words are the last trip's unless step A resets them -- then a damaged
    block, then valid ones; at 32,768 a full block, then a tiny one inside its leftovers"""
    trips = {t[0]: t for t in wc.trips()}
    for bs in (700, 4097):
        name, stream, offs, total, size, blocks = trips["trip-bs%d" % bs]
        assert size == bs and 3 <= len(blocks) <= 6 and total == sum(n for _, n in blocks) and len(offs) == len(blocks)
        for waves in (2, 16):
            ms = [wc.model(body, n, waves) for body, n in blocks]
            entered = [s for s, sh in enumerate(ms[0].shares) if sh]
            assert len(entered) >= 2 and len(ms[0].passed) <= 1 and ms[0].valid
            assert ms[1].valid and len(ms[1].passed) == -(-ms[1].csz // ms[1].share) - 1 >= 1 and set(ms[1].passed) & set(entered)
            assert len(ms[1].elements) == 1
            assert [m.valid for m in ms[2:]] == [False] + [True] * (len(ms) - 3)
            assert all(m.within for m in ms)
    name, stream, offs, total, size, blocks = trips["trip-bs32768"]
    ms = [wc.model(body, n, 16) for body, n in blocks]
    assert size == wc.WIDE_MAX_BLOCK and len(blocks) == 2 and ms[0].out_len == size and ms[1].out_len < 64
    assert ms[0].valid and ms[1].valid and ms[0].rounds >= 10 and ms[1].hops > 0 and ms[0].csz > 64 * 16 > ms[1].csz
    for t in wc.trips():
        total, bs, offs = kc._offsets(t[1])
        assert (total, bs, offs) == (t[3], t[4], t[2])


def test_the_small_containers_meet_every_alignment_of_a_17_byte_window():
    conts = wc.small_containers()
    assert [c[5] for c in conts] == [17, 1, 15, 16, 31, 33, 48]
    name, stream, plain, offs, total, bs = conts[0]
    assert len(offs) == 100 and {(k * bs) & 15 for k in range(len(offs))} == set(range(16))
    for name, stream, plain, offs, total, bs in conts:
        for k, at in enumerate(offs):
            n = min(bs, total - k * bs)
            m = wc.job_model((name, stream, at, n), 16)
            assert m.valid and m.out == plain[k * bs:k * bs + n] and m.words == wc.WIDE, (name, k)
