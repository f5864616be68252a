"""Blocks aimed at the seams between the two window loops of k2_decode_block (csrc/snappy_kernels.hpp): the STEADY loop takes
the interior windows -- base g with g + 64 <= csz and g + 200 <= avail, avail = the stream's bytes from the block's first
element on -- the COLD loop every other one.  Shared by tests/test_k2_steady_emulated.py (every block decoded alone between
inaccessible pages) and tests/test_gpu_k2_steady.py (between guard bytes).  Test infrastructure only: plain Python + the oracle.

A job is k2_window_cases' (name, stream, at, out_len) and is judged by its rule (check_job: K2 may reject what the oracle
accepts, never the other way round, accepted bytes are equal) and by its name: "valid ..." must be accepted, "defect ..."
must be rejected.  raw_items() gives the same bodies as raw Snappy streams (the size word stripped, the header of their
output length in front) for k2_decode_block<true>."""
import k2_window_cases as kc
import raw_cases as rc

# compressed sizes around the interior boundary: one window, two, the first size with an interior window when the block ends
# the stream (200) and its neighbours, the sizes at which the second and third interior window appear
SIZES = (63, 64, 65) + tuple(range(127, 130)) + tuple(range(191, 202)) + tuple(range(255, 266)) + tuple(range(327, 330))
FOLLOW = (0, 8, 71, 72, 73, 200)        # bytes of a following block behind the block (0: the block ends the stream)
ATS = tuple(range(8, 16))               # the size word's offset in the stream: 0-7 mod 8


def steady_end(csz, avail):
    """the model of k2_decode_block's steady_end: window bases below it are interior"""
    if csz < 64 or avail < 200:
        return 0
    return (min(csz - 64, avail - 200) & ~63) + 64


def body_of(c, salt=0):
    """-> (exactly c compressed bytes of literals of at most 60, their output length); c >= 2.  61 compressed bytes a literal,
    so element starts meet every window alignment."""
    assert c >= 2
    out, n = b"", 0
    while c:
        step = min(61, c)
        if c - step == 1:
            step -= 1
        out += kc._literal(kc._payload(step - 1, n + salt))
        n += step - 1
        c -= step
    return out, n


def _following(n):
    nb, _ = body_of(300, 77)
    return (len(nb).to_bytes(4, "little") + nb)[:n]


def frame(name, body, out_len, at, follow):
    stream = kc._payload(at, 5) + len(body).to_bytes(4, "little") + body + _following(follow)
    return ("%s at=%d follow=%d" % (name, at, follow), stream, at, out_len)


def _run_on_literal(tagpos, end):
    """a literal whose tag is at compressed offset tagpos and whose payload ends (exclusively) at `end`"""
    for lb in (0, 1, 2):                # length bytes behind the tag: the first form that holds the length
        n = end - tagpos - 1 - lb
        if 1 <= n <= (60, 256, 65536)[lb]:
            return kc._literal(kc._payload(n, tagpos), lb)
    raise AssertionError((tagpos, end))


def size_bodies():
    return [("valid csz=%d" % c,) + body_of(c) for c in SIZES]


def run_on_bodies():
    """(name, body, out_len): from the steady window at g = 128, a literal that ends at g + 127 (the loop stays), g + 128 and
    g + 129 (it leaves and the cold loop loads afresh), g + 5000; behind it 400 bytes (the next window is interior: the block
    re-enters the steady loop) or 10 (it is not)."""
    v = []
    g = 128
    for tag_lane in (0, 20, 63):
        prefix, n0 = body_of(g + tag_lane)
        for end in (g + 127, g + 128, g + 129, g + 5000):
            lit = _run_on_literal(g + tag_lane, end)
            assert len(prefix) + len(lit) == end
            for rest in (400, 10):
                suffix, n2 = body_of(rest, 3)
                v.append(("valid literal from lane %d ends at g+%d, %d bytes behind" % (tag_lane, end - g, rest),
                          prefix + lit + suffix, n0 + _literal_output(lit) + n2))
    return v


def _literal_output(lit):
    tag = lit[0] >> 2
    return tag + 1 if tag < 60 else int.from_bytes(lit[1:1 + tag - 59], "little") + 1


DEFECT_CSZ = 360            # five full windows and a partial one: with 200 bytes behind the block the steady loop takes 0 .. 4


def defect_bodies():
    """(name, body, out_len): each defect in window 0, 2 and 4 of a block of DEFECT_CSZ compressed bytes -- with 200 bytes behind
    the block the first, a middle and the last window of the steady loop (with none: the first, the last, and one the cold loop
    takes).  The defect is the last element that starts in its window (at lane 61); literals in front of it and behind."""
    v = []
    for w in (0, 2, 4):
        p = 64 * w + 61
        prefix, op = body_of(p)

        def whole(defect, salt=w):
            suffix, n = body_of(DEFECT_CSZ - p - len(defect), salt)
            return prefix + defect + suffix, n

        body, n = whole(bytes([62 << 2, 0, 0, 1]))
        v.append(("defect w=%d an element predecode rejects" % w, body, op + n + 7))
        body, n = whole(kc._copy2(4, 1))
        v.append(("valid w=%d a copy of 4 at lane 61" % w, body, op + 4 + n))
        v.append(("defect w=%d op + total one past out_len" % w, body, op + 3))
        body, n = whole(kc._copy2(4, 0))
        v.append(("defect w=%d copy with offset 0" % w, body, op + 4 + n))
        body, n = whole(kc._copy2(4, op))
        v.append(("valid w=%d copy with offset dstp" % w, body, op + 4 + n))
        body, n = whole(kc._copy2(4, op + 1))
        v.append(("defect w=%d copy with offset dstp + 1" % w, body, op + 4 + n))
        # 22 copies of 64: the most a window can produce.  Window 0 needs a byte to copy from: 21 of them start in it.
        if w == 0:
            front, op22, in_window = kc._fill(1), 1, 21
        else:
            front, op22 = body_of(64 * w)
            in_window = 22
        copies = kc._copy2(64, 1) * 22
        suffix, n = body_of(DEFECT_CSZ - len(front) - len(copies), 9)
        v.append(("valid w=%d 22 copies of 64" % w, front + copies + suffix, op22 + 22 * 64 + n))
        v.append(("defect w=%d 22 copies of 64, the window's output one past out_len" % w, front + copies + suffix,
                  op22 + in_window * 64 - 1))
    return v


def hand_jobs():
    jobs = []
    for name, body, n in size_bodies():
        for follow in FOLLOW:
            for at in ATS:
                jobs.append(frame(name, body, n, at, follow))
    for name, body, n in run_on_bodies() + defect_bodies():
        for follow in (0, 200):
            jobs.append(frame(name, body, n, 8 + len(jobs) % 8, follow))
    return jobs


def intact_jobs():
    """every block of datagen.element_stream flavours 0-3 at block sizes 64, 700, 4097 and 32768 (k2_window_cases' containers)"""
    return [j for j in kc.intact_jobs() if "-bs65535-" not in j[0]]


def raw_items():
    """[(name, raw stream, capacity)]: every hand-made body once, as a raw Snappy stream of its own"""
    return [(name, rc.varint(n) + body, n) for name, body, n in size_bodies() + run_on_bodies() + defect_bodies()]


def judge(job, st, out):
    """-> problem text or None for K2's answer (st, out bytes) to one job"""
    name = job[0]
    p = kc.check_job(job, st, out)
    if p is None and st != 0 and (name.startswith("valid ") or kc.must_accept(job)):
        p = name + ": a valid block was rejected"
    if p is None and st == 0 and name.startswith("defect "):
        p = name + ": a block with a defect was accepted"
    return p


def judge_raw(item, st, out_len, window):
    """the same rule for one raw item: `window` = its capacity bytes after the call"""
    name, s, n = item
    want_st, want_n, plain = rc.expect(s, n)
    if st not in (rc.OK, rc.INVALID) or out_len != n:
        return "%s: status %r, length %r" % (name, st, out_len)
    if st == rc.OK and (want_st != rc.OK or window[:n] != plain):
        return "%s: accepted, and the format's CPU statement says %r" % (name, want_st)
    if st != rc.OK and name.startswith("valid "):
        return name + ": a valid stream was rejected"
    if st == rc.OK and name.startswith("defect "):
        return name + ": a stream with a defect was accepted"
    return None
