"""Cases for the wide block decoder (csrc/snappy_k2_wide.hpp; tests/test_k2_wide_emulated.py on the wave emulator,
tests/test_gpu_k2_wide.py on the GPU).  Test infrastructure only: plain Python + the oracle.

A job is k2_window_cases' (name, stream, at, out_len): the block whose u32 size word is at stream[at], decoded alone into
out_len bytes.  The yardsticks are K2 itself on the same job (status, and bytes where the status is OK) and the oracle
(k2_window_cases.check_job); the result words follow from K2's status and the limits alone (expected_result).

The second half of the file is a MODEL of the kernel's steps in plain Python (model) and generators of small blocks aimed at
the shares, the windows and the copy chains; tests/test_k2_wide_model.py holds the generators to their coverage conditions by
the model alone, and the model's verdict, bytes and result words are a third yardstick for those blocks."""
import os

import datagen
import k2_window_cases as kc
import oracle_lib as oracle

WIDE_MAX_BLOCK = 32768            # SNAPPY_HIP_WIDE_MAX_BLOCK
WIDE_MAX_CSZ = 38400              # SNAPPY_HIP_WIDE_MAX_CSZ
assert WIDE_MAX_CSZ >= 32 + 32768 + 32768 // 6
WAVES = (2, 16)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def within(stream, at, out_len):
    """is the block at `at` inside the wide path's limits?"""
    if out_len > WIDE_MAX_BLOCK or at + 4 > len(stream):
        return False
    csz = int.from_bytes(stream[at:at + 4], "little")
    return csz <= WIDE_MAX_CSZ and at + 4 + csz <= len(stream)


def expected_result(blocks):
    """blocks: (within the limits?, K2's status) per block -> the four result words"""
    return [sum(1 for w, st in blocks if w and st == 0), sum(1 for w, _ in blocks if not w), sum(1 for w, st in blocks if w and st != 0), 0]


def share_bytes(csz, waves):
    """the compressed bytes of one share (csrc/snappy_k2_wide.hpp, step B)"""
    per = (csz + waves - 1) // waves
    return (per + 63) & ~63 if per > 64 else 64


# ---- hand-built blocks aimed at what is new ----------------------------------------------------------------------------

def _copy1(length, offset):
    assert 4 <= length <= 11 and offset < 2048
    return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 0xff])


def _copy4(length, offset):
    return bytes([3 | ((length - 1) << 2)]) + offset.to_bytes(4, "little")


def _exact_fill(nbytes, salt=0):
    """literals of at most 60 bytes that take exactly nbytes compressed bytes -> (body, output bytes)"""
    body, out, n = b"", 0, nbytes
    assert n != 1
    while n > 0:
        step = min(61, n)
        if n - step == 1:
            step -= 1
        body += kc._literal(kc._payload(step - 1, salt + out))
        out += step - 1
        n -= step
    assert len(body) == nbytes
    return body, out


def _straddle(waves, boundary, lit_len, tag_before, csz):
    """a block of csz compressed bytes whose shares are `boundary` bytes at `waves` wavefronts, with a literal of lit_len bytes
    whose tag lies tag_before bytes in front of the first share boundary -> (body, out_len)"""
    head, o1 = _exact_fill(boundary - tag_before, 1)
    lit = kc._literal(kc._payload(lit_len, 77))
    tail, o2 = _exact_fill(csz - len(head) - len(lit), 5)
    body = head + lit + tail
    assert len(body) == csz and share_bytes(csz, waves) == boundary and len(head) + len(lit) > boundary
    return body, o1 + lit_len + o2


def hand_bodies():
    """(name, compressed body, out_len); names that start with "valid" must be accepted"""
    v = []
    v.append(("valid shorter than the shares", kc._fill(100), 100))                       # 102 bytes: most shares are empty
    for L in (1, 63, 64, 65, 32768):
        v.append(("valid literals out_len=%d" % L, kc._fill(L), L))
    for waves, boundary, csz in ((2, 640, 1270), (16, 640, 10000)):
        # a 62-byte literal (64 compressed bytes) from the boundary's last byte on: the next entry is byte 63 of the share
        body, L = _straddle(waves, boundary, 62, 1, csz)
        v.append(("valid literal 62 straddles a share of W=%d" % waves, body, L))
        # ... and a 5,000-byte one: the next entry lies behind the share's first 64 bytes (W = 16: behind whole shares)
        if waves == 16:
            body, L = _straddle(waves, boundary, 5000, 10, csz)
            v.append(("valid literal 5000 straddles a share of W=%d" % waves, body, L))
    body, L = _straddle(2, 5056, 5000, 10, 10100)
    v.append(("valid literal 5000 straddles a share of W=2", body, L))
    v.append(("valid literal covers two whole shares", kc._fill(10) + kc._literal(kc._payload(300)) + kc._fill(50), 360))
    v.append(("valid deepest chain", kc._literal(b"x") + kc._copy2(64, 1) * 511 + kc._copy2(63, 1), 32768))
    v.append(("valid copy offset == op", kc._fill(10) + kc._copy2(10, 10), 20))
    v.append(("copy offset == op + 1", kc._fill(10) + kc._copy2(10, 11), 20))
    v.append(("copy offset 0", kc._fill(10) + kc._copy2(10, 0), 20))
    v.append(("valid overlapping copies", kc._fill(5) + kc._copy2(40, 3) + kc._copy2(17, 2) + kc._fill(9) + kc._copy2(64, 7), 135))
    v.append(("valid 22 copies of 64 in one window", kc._fill(1) + kc._copy2(64, 1) * 22, 1 + 22 * 64))
    four = kc._fill(70) + _copy1(11, 70) + kc._copy2(33, 81) + _copy4(64, 100) + kc._literal(kc._payload(61), 2) + _copy1(4, 1)
    v.append(("valid all four element types", four, 70 + 11 + 33 + 64 + 61 + 4))
    v.append(("valid all four element types, twice over", four + four, 2 * 243))
    n = 19300                                                                             # 38,600 compressed bytes
    v.append(("valid 1-byte literals beyond the csz limit", b"".join(bytes([0, (i * 5) & 0xff]) for i in range(n)), n))
    v.append(("output one short of out_len", kc._fill(99), 100))
    v.append(("output one past out_len", kc._fill(101), 100))
    return v


def hand_jobs():
    jobs = []
    for name, body, L in hand_bodies():
        stream = kc._varint(L) + kc._varint(L) + len(body).to_bytes(4, "little") + body
        at = len(stream) - 4 - len(body)
        jobs.append(("wide %s" % name, stream + kc._payload(40, 9), at, L))
        jobs.append(("wide %s (block ends the stream)" % name, stream, at, L))
    # a size word that leaves the stream: the payload is cut short, and the size word itself is
    body = kc._fill(200)
    stream = kc._varint(200) + kc._varint(200) + len(body).to_bytes(4, "little") + body
    at = len(stream) - 4 - len(body)
    jobs.append(("wide payload leaves the stream", stream[:-1], at, 200))
    jobs.append(("wide size word leaves the stream", stream[:at + 3], at, 200))
    jobs.append(("wide offset behind the stream", stream, len(stream) + 5, 200))
    return jobs


def must_accept(job):
    return job[0].startswith("wide valid") or kc.must_accept(job)


# every compressor-made or valid-by-construction job of at most 32 KiB stays within the csz limit: the wide path must take it
for _job in kc.intact_jobs():
    assert _job[3] > WIDE_MAX_BLOCK or within(_job[1], _job[2], _job[3]), _job[0]


# ---- whole containers --------------------------------------------------------------------------------------------------

def golden(name):
    with open(os.path.join(GOLDEN, name + ".snappy"), "rb") as f:
        stream = f.read()
    with open(os.path.join(GOLDEN, name + ".txt"), "rb") as f:
        return stream, f.read()


def containers(goldens=("terror2", "alice", "coding")):
    """(name, stream, plaintext, offsets, total_len, block_size)"""
    out = []
    for name in goldens:
        stream, plain = golden(name)
        out.append((name, stream, plain))
    for flavour in range(4):
        for k, bs in enumerate((700, 4097, 32768)):
            total = 3 * bs + 17 + k if bs <= 4097 else bs + 3000 + 501 * k
            stream, plain = datagen.element_stream(total, bs, 7100 + 10 * flavour + k, flavour)
            out.append(("elem-f%d-bs%d" % (flavour, bs), stream, plain))
    full = []
    for name, stream, plain in out:
        total, bs, offs = kc._offsets(stream)
        assert total == len(plain)
        full.append((name, stream, plain, offs, total, bs))
    return full


def serial_container():
    """block size 65,535: every block goes to the serial decoder"""
    stream, plain = datagen.element_stream(2 * 65535 + 1234, 65535, 7177, 1)
    total, bs, offs = kc._offsets(stream)
    return ("elem-f1-bs65535", stream, plain, offs, total, bs)


# ---- the model: one serial walk of a block's compressed body -------------------------------------------
# It shares no code with the kernel or the emulator.  What it says of a block is what steps B-E of k2_wide_kernel must make of
# it; the generators below are judged by it alone (tests/test_k2_wide_model.py), so they cannot quietly stop covering a case.

ALL_WAVES = (2, 4, 8, 16)
WIDE, BEYOND, UNPROVEN = [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]
LITERAL = 0


class Element:
    """pos: the tag's position in the body; type: 0 literal, 1 / 2 / 3 copy with a 1-, 2-, 4-byte offset; hdr: header bytes;
    olen: output bytes; off: a copy's offset (None for a literal); op: where its output starts"""

    def __init__(self, pos, type_, hdr, olen, off, op):
        self.pos, self.type, self.hdr, self.olen, self.off, self.op = pos, type_, hdr, olen, off, op
        self.size = hdr + (olen if type_ == LITERAL else 0)

    @property
    def kind(self):
        return "literal%d" % self.hdr if self.type == LITERAL else "copy%d" % (1, 2, 4)[self.type - 1]


class Model:
    pass


def _sized(body):
    """the element chain by sizes alone, as predecode judges it -> (elements, True if it ends exactly on csz)"""
    els, pos, op, csz = [], 0, 0, len(body)
    while pos < csz:
        tag = body[pos]
        t, v = tag & 3, tag >> 2
        if t == LITERAL:
            hdr = 1 if v < 60 else v - 58
            field = v if v < 60 else int.from_bytes(body[pos + 1:pos + hdr], "little")
            if pos + hdr > csz or field >= 65536:
                return els, False
            olen, off = field + 1, None
        else:
            hdr = (2, 3, 5)[t - 1]
            if pos + hdr > csz:
                return els, False
            olen = (v & 7) + 4 if t == 1 else v + 1
            off = ((tag >> 5) << 8) | body[pos + 1] if t == 1 else int.from_bytes(body[pos + 1:pos + hdr], "little")
        e = Element(pos, t, hdr, olen, off, op)
        if pos + e.size > csz:
            return els, False
        els.append(e)
        pos += e.size
        op += olen
    return els, True


def model(body, out_len, waves):
    """What the wide decoder must make of one block at `waves` wavefronts:
    valid / out            K2's verdict (predecode's rejections, output past out_len, a copy with offset 0 or reaching before byte
                           0, output short of out_len) and the model's own decode
    elements               Element per element of the size chain
    within / words         the limits, and the result words of a one-block call
    share / shares         the share size and per share None (not entered) or a dict: entry, base, landing, end, table (step C
                           reads the entry from the table: offset < 64) and offset = entry - the share's first byte
    passed                 the shares in front of csz that the chain passes over
    windows                per 64-byte window of every share's walk a dict: share, g, elements, and for a last literal that
                           runs on: runon = dict(lane, hdr, ps, frm, n, branch, passes, ending)
    hops / rounds          step E's deepest source chain and ceil(log2(hops)), 0 without copies
    cross_literal / cross_copy / cross_depth
                           a copy reads bytes another share's literal / another share's copy made; the most share-to-share
                           copy links in one byte's chain"""
    m = Model()
    m.csz, m.out_len, m.waves = len(body), out_len, waves
    m.within = out_len <= WIDE_MAX_BLOCK and m.csz <= WIDE_MAX_CSZ
    m.elements, sized = _sized(body)
    out, ok = bytearray(), sized
    for e in m.elements:
        if not ok:
            break
        if e.olen > out_len - len(out) or (e.type != LITERAL and (e.off == 0 or e.off > len(out))):
            ok = False
        elif e.type == LITERAL:
            out += body[e.pos + e.hdr:e.pos + e.size]
        else:
            for _ in range(e.olen):
                out.append(out[-e.off])
    m.valid = ok and len(out) == out_len
    m.out = bytes(out) if m.valid else None
    m.words = BEYOND if not m.within else (WIDE if m.valid else UNPROVEN)
    m.share = share = share_bytes(m.csz, waves)
    m.shares, m.passed, m.windows = [None] * waves, [], []
    m.hops = m.rounds = m.cross_depth = 0
    m.cross_literal = m.cross_copy = False
    if not sized:
        return m
    starts = [e.pos for e in m.elements] + [m.csz]
    bases = [e.op for e in m.elements] + [sum(e.olen for e in m.elements)]
    for s in range(waves):
        start, limit = s * share, min((s + 1) * share, m.csz)
        if start >= m.csz:
            break
        k = next((k for k, p in enumerate(starts[:-1]) if start <= p < limit), None)
        if k is None:
            m.passed.append(s)
            continue
        j = next(j for j in range(k, len(starts)) if starts[j] >= limit)
        m.shares[s] = dict(entry=starts[k], base=bases[k], landing=starts[j], end=bases[j], offset=starts[k] - start,
                           table=starts[k] - start < 64, first=k, beyond=j)
        cp = k
        while cp < j:                                                   # the windows of this share's walk
            g = starts[cp] & ~63
            wend = min(limit, g + 64)
            nxt = next(i for i in range(cp, len(starts)) if starts[i] >= wend)
            w = dict(share=s, g=g, elements=m.elements[cp:nxt], runon=None)
            last = m.elements[nxt - 1]
            s_end = last.pos + last.size - g
            if s_end > 64 and last.type == LITERAL:
                lane = last.pos - g
                ps = lane + last.hdr
                frm = max(ps, 64)
                n = s_end - frm
                ending = "last" if nxt == len(m.elements) else ("literal" if m.elements[nxt].type == LITERAL else "copy")
                w["runon"] = dict(lane=lane, hdr=last.hdr, ps=ps, frm=frm, n=n, passes=-(-n // 256) if n >= 4 else 1,
                                  branch="n<4" if n < 4 else "n>=4 mod %d" % (n % 4), ending=ending)
            m.windows.append(w)
            cp = nxt
    if not m.valid:
        return m
    # step E: every output byte's chain back to a literal's byte
    n_out = out_len
    owner, depth, xdepth = [0] * n_out, [0] * n_out, [0] * n_out
    share_of = [e.pos // share for e in m.elements]
    for k, e in enumerate(m.elements):
        for i in range(e.op, e.op + e.olen):
            owner[i] = k
            if e.type != LITERAL:
                src = i - e.off
                depth[i] = depth[src] + 1
                p = owner[src]
                other = share_of[p] != share_of[k]
                if other and m.elements[p].type == LITERAL:
                    m.cross_literal = True
                if other and m.elements[p].type != LITERAL:
                    m.cross_copy = True
                    xdepth[i] = xdepth[src] + 1
                else:
                    xdepth[i] = xdepth[src]
    m.hops = max(depth) if depth else 0
    m.rounds = (m.hops - 1).bit_length() if m.hops else 0
    m.cross_depth = max(xdepth) if xdepth else 0
    return m


def job_body(job):
    """the compressed body of a job's block, or None where the size word or the body leaves the stream"""
    _, stream, at, _ = job
    if at + 4 > len(stream):
        return None
    csz = int.from_bytes(stream[at:at + 4], "little")
    return stream[at + 4:at + 4 + csz] if at + 4 + csz <= len(stream) else None


def job_model(job, waves):
    body = job_body(job)
    return None if body is None else model(body, job[3], waves)


# ---- generators: small blocks, valid by construction unless their name says otherwise ---------------------------------------
# A block is (name, body, out_len, waves): `waves` is the workgroup size whose shares it is aimed at (None: any).  Names that
# start with "valid" must be accepted.  Every generator is deterministic.

ENTRY_OFFSETS = (0, 1, 2, 3, 4, 61, 62, 63, 64, 65, 127, 128, 129)
RUNON_N = (1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 257, 300)
LITERAL_CAP = {1: 60, 2: 256, 3: 65536, 4: 65536, 5: 65536}          # the longest payload a header of that many bytes can state


def _lit(n, hdr=None, salt=0):
    """a literal of n bytes with `hdr` header bytes (None: the shortest)"""
    return kc._literal(kc._payload(n, salt), None if hdr is None else hdr - 1)


def _copy(kind, length, offset):
    return {1: _copy1, 2: kc._copy2, 4: _copy4}[kind](length, offset)


def sweep_share(waves):
    """the share size of the boundary sweep's blocks: every entry offset up to 129 fits a share, but for W = 16, whose blocks
    stay near 2 KiB (there offsets 128 and 129 are offsets 0 and 1 of the share after a share passed over)"""
    return 128 if waves == 16 else 192


def boundaries(waves):
    """(which, share index) of the first, a middle and the last share boundary"""
    seen = {}
    for which, si in (("first", 1), ("last", waves - 1), ("middle", waves // 2)):
        seen.setdefault(si, which)
    return sorted(((which, si) for si, which in seen.items()), key=lambda b: b[1])


def _around(waves, share, pos, element, salt=0):
    """a block of `waves` shares of `share` bytes with `element` at byte `pos` between literal fills, or None if it cannot be
    -> (body, output bytes in front of the element, output bytes behind it)"""
    end = pos + len(element)
    if end > waves * share:
        return None
    csz = max(waves * share - 7, end)
    if csz - end == 1:
        csz += 1
        if csz > waves * share:
            return None
    head, o1 = _exact_fill(pos, 1 + salt)
    tail, o2 = _exact_fill(csz - end, 5 + salt)
    body = head + element + tail
    assert share_bytes(len(body), waves) == share and len(body) > (waves - 1) * share
    return body, o1, o2


def boundary_blocks(waves):
    """every element kind with its tag d = 0 .. header bytes in front of the first, a middle and the last share boundary;
    literals in every payload length that puts the next element at one of ENTRY_OFFSETS behind the boundary"""
    share, v = sweep_share(waves), []
    for which, si in boundaries(waves):
        b = si * share
        for hdr in (1, 2, 3, 4, 5):
            for d in range(hdr + 1):
                for t in ENTRY_OFFSETS:
                    n = t - hdr + d
                    if not 1 <= n <= LITERAL_CAP[hdr]:
                        continue
                    made = _around(waves, share, b - d, _lit(n, hdr, 11 * d + t), t)
                    if made:
                        v.append(("valid %s boundary W=%d literal%d d=%d next at %d" % (which, waves, hdr, d, t), made[0], made[1] + n + made[2], waves))
        for kind, hdr in ((1, 2), (2, 3), (4, 5)):
            for d in range(hdr + 1):
                length = (4 + d, 64 - 9 * d, 1 + 12 * d)[(1, 2, 4).index(kind)]
                body, o1, o2 = _around(waves, share, b - d, _copy(kind, length, 1 + 17 * d + hdr), d)
                v.append(("valid %s boundary W=%d copy%d d=%d" % (which, waves, kind, d), body, o1 + length + o2, waves))
    return v


def long_literal_blocks(waves):
    """literals that pass over 1 share, 2 shares and all the remaining ones (W >= 4), and one from share 0 to csz"""
    share, v = sweep_share(waves), []
    for hdr, skip in ((3, 1), (4, 2)) if waves >= 4 else ():
        n = (1 + skip) * share + 5 - 70 - hdr                            # from byte 70 to byte 5 of share 1 + skip
        body, o1, o2 = _around(waves, share, 70, _lit(n, hdr, skip))
        v.append(("valid literal passes over %d shares W=%d" % (skip, waves), body, o1 + n + o2, waves))
    for start in (70,) + ((share + 70,) if waves >= 4 else ()):
        head, o1 = _exact_fill(start, 3)
        n = waves * share - 9 - start - 3
        v.append(("valid literal from byte %d to csz W=%d" % (start, waves), head + _lit(n, 3, 9), o1 + n, waves))
    return v


def _in_last_share(lane, element, follow):
    """a block for two wavefronts with `element`'s tag at `lane` of a window of the last share, `follow` behind it"""
    g = 64
    while share_bytes(g + lane + len(element) + len(follow), 2) > g:
        g += 64
    head, o1 = _exact_fill(g + lane, 2)
    return head + element + follow, o1


def window_blocks():
    """inside one share (W = 2): a literal's tag at lanes 56..63 of a window, every header length, run-ons of RUNON_N bytes,
    as the block's last element and followed by a literal or a copy; copies with 2, 3 and 5 header bytes at lanes 59..63"""
    v = []
    follows = (("last", b"", 0), ("literal", _lit(3, None, 40), 3), ("copy", kc._copy2(5, 2), 5))
    for lane in range(56, 64):
        for hdr in (1, 2, 3, 4, 5):
            for n in RUNON_N:
                ps = lane + hdr
                length = n if ps > 64 else n + 64 - ps
                if not 1 <= length <= LITERAL_CAP[hdr]:
                    continue
                for ending, follow, o2 in follows:
                    body, o1 = _in_last_share(lane, _lit(length, hdr, lane + n), follow)
                    v.append(("valid window lane %d literal%d run-on %d then %s" % (lane, hdr, n, ending), body, o1 + length + o2, 2))
    for lane in range(59, 64):
        for kind, length in ((1, 11), (2, 64), (4, 1)):
            for ending, follow, o2 in follows[:2]:
                body, o1 = _in_last_share(lane, _copy(kind, length, 3 + lane), follow)
                v.append(("valid window lane %d copy%d then %s" % (lane, kind, ending), body, o1 + length + o2, 2))
    return v


def chain_blocks():
    """copy chains for step E: exactly r rounds of doubling for r = 0..15 (one literal byte, then copies at offset 1 up to
    2^r + 1 bytes, the last ones up to 32,768), and overlapping copies at every offset 1..8 in every length 1..64"""
    v = []
    for r in range(16):
        total = min((1 << r) + 1, WIDE_MAX_BLOCK)
        full, rest = divmod(total - 1, 64)
        body = _lit(1) + kc._copy2(64, 1) * full + (kc._copy2(rest, 1) if rest else b"")
        v.append(("valid chain of %d rounds" % r, body, total, None))
    for off in range(1, 9):
        body = _lit(8, None, off) + b"".join(kc._copy2(n, off) for n in range(1, 65))
        v.append(("valid overlapping copies at offset %d" % off, body, 8 + 64 * 65 // 2, None))
    return v


def cross_share_blocks(waves):
    """copies whose source is a literal of an earlier share, and copies whose source is an earlier share's copy, chained from
    share to share; as every later share's first element a copy that reaches byte 0 exactly (valid), one byte before it and
    a copy with offset 0 (both invalid: step D judges them with the base step C handed over)"""
    share, v = 128, []
    body, op = _exact_fill(share, 4)
    b_at = 20                                                            # where the chained copy's source starts
    for s in range(1, waves):
        body += kc._copy2(9, op - 3)                                     # from share 0's literal
        op += 9
        body += kc._copy2(12, op - b_at)                                 # from the last share's chained copy (share 1: a literal)
        b_at = op
        op += 12
        fill, o = _exact_fill(share - 6 - (7 if s == waves - 1 else 0), s)
        body += fill
        op += o
    assert share_bytes(len(body), waves) == share
    v.append(("valid copies from earlier shares W=%d" % waves, body, op, waves))
    for s in range(1, waves):
        head, dstp = _exact_fill(s * share, 6)
        tail, o2 = _exact_fill((waves - s) * share - 3 - 7, 8)
        for name, off in (("valid first copy of share %d reaches byte 0" % s, dstp), ("first copy of share %d reaches before byte 0" % s, dstp + 1),
                          ("first copy of share %d has offset 0" % s, 0)):
            v.append(("%s W=%d" % (name, waves), head + kc._copy2(10, off) + tail, dstp + 10 + o2, waves))
    return v


def bound_blocks(waves):
    """the output bound in the first, a middle and the last share: one literal there a byte longer or shorter than out_len
    has room for (the block's output one past / one short), and out_len one less than the output up to and with it"""
    share, v = 128, []
    for which, si in sorted({0: "first", waves // 2: "middle", waves - 1: "last"}.items()):
        which, si = si, which
        head, o1 = _exact_fill(si * share, 2)
        tail, o2 = _exact_fill((waves - si) * share - 31 - 9, 3) if si < waves - 1 else (b"", 0)
        for name, n, out_len in (("output one past out_len", 31, o1 + 30 + o2), ("output one short of out_len", 29, o1 + 30 + o2),
                                 ("output passes out_len by one byte", 30, o1 + 29)):
            if name.endswith("by one byte") and si == waves - 1:
                continue                                                 # (the last share's is "one past")
            v.append(("%s in the %s share W=%d" % (name, which, waves), head + _lit(n, None, si) + tail, out_len, waves))
        v.append(("valid output meets out_len, %s share W=%d" % (which, waves), head + _lit(30, None, si) + tail, o1 + 30 + o2, waves))
    return v


def limit_blocks():
    """csz 0, csz at and one past the limit (both valid), and a run-on literal that ends exactly at out_len 32,768"""
    ones = b"".join(bytes([0, (i * 5) & 0xff]) for i in range(19200))
    head, o1 = _exact_fill(64 + 60, 1)
    return [("no compressed bytes at all", b"", 1, None),
            ("valid csz at the limit", ones, 19200, None),
            ("valid csz one past the limit", ones[:-2] + _lit(2, None, 1), 19201, None),
            ("valid run-on literal ends at out_len 32768", head + _lit(WIDE_MAX_BLOCK - o1, 4, 6), WIDE_MAX_BLOCK, None)]


def small_blocks():
    """every generated block but the few large ones (limit_blocks, the longest chains)"""
    v = window_blocks() + [b for b in chain_blocks() if b[2] <= 4096]
    for waves in ALL_WAVES:
        v += boundary_blocks(waves) + long_literal_blocks(waves) + cross_share_blocks(waves) + bound_blocks(waves)
    assert all(len(b[1]) <= 2200 and b[2] <= 4096 for b in v)
    return v


def large_blocks():
    return [b for b in chain_blocks() if b[2] > 4096] + limit_blocks()


def block_jobs(blocks):
    """the blocks as jobs of k2_window_cases' kind; every other one with bytes behind it that a decoder running on would pick up"""
    jobs = []
    for k, (name, body, L, _) in enumerate(blocks):
        stream = kc._varint(L) + kc._varint(L) + len(body).to_bytes(4, "little") + body
        jobs.append(("wide " + name, stream + (kc._payload(40, 9) if k % 2 else b""), len(stream) - 4 - len(body), L))
    return jobs


# ---- trips: containers one workgroup decodes block after block -------------------------------------------------------------

def _busy_block(out_len, salt):
    """out_len bytes from short literals and copies of every type: many elements, every share entered"""
    body, op, k = b"", 0, salt
    while op < out_len:
        left = out_len - op
        k += 1
        if op < 70 or k % 3 == 0:
            n = min(left, 1 + (k * 7) % 40)
            body += _lit(n, None, k)
        elif k % 3 == 1:
            n = min(left, 1 + (k * 11) % 64)
            body += kc._copy2(n, 1 + (k * 5) % 64)
        else:
            n = min(left, 4 + k % 8)
            body += _copy1(n, 1 + (k * 13) % 60) if n >= 4 else _copy4(n, 2)
        op += n
    return body


def trips():
    """(name, stream, offsets, total_len, block_size, [(body, out_len)]): at block sizes 700 and 4,097 a block that enters
    many shares, one long literal (most shares passed over), a damaged block, valid blocks; at 32,768 a full block and a tiny
    last one.  Whatever a trip leaves in LDS meets the next block."""
    v = []
    for bs in (700, 4097):
        busy = _busy_block(bs, bs)
        copies = [e for e in _sized(busy)[0] if e.type == 2]
        hit = copies[len(copies) // 2]                                   # a copy in the block's middle gets offset 0
        damaged = busy[:hit.pos + 1] + b"\0\0" + busy[hit.pos + 3:]
        blocks = [(busy, bs), (_lit(bs, 3, 1), bs), (damaged, bs), (_busy_block(bs, 9), bs), (_lit(bs, 5, 2), bs), (_busy_block(333, 4), 333)]
        v.append(("trip-bs%d" % bs, blocks, bs))
    full = _lit(1) + kc._copy2(64, 1) * 100 + _busy_block(WIDE_MAX_BLOCK - 6401, 1)
    v.append(("trip-bs32768", [(full, WIDE_MAX_BLOCK), (_lit(5, None, 3) + kc._copy2(6, 2), 11)], WIDE_MAX_BLOCK))
    out = []
    for name, blocks, bs in v:
        total = sum(n for _, n in blocks)
        stream, offs = kc._varint(total) + kc._varint(bs), []
        for body, _ in blocks:
            offs.append(len(stream))
            stream += len(body).to_bytes(4, "little") + body
        out.append((name, stream, offs, total, bs, blocks))
    return out


def small_containers():
    """(name, stream, plaintext, offsets, total_len, block_size): 100 blocks of 17 bytes -- with step F's head, middle and tail
    every alignment of a block's window against out_len 17 -- and block sizes 1, 15, 16, 31, 33 and 48"""
    out = []
    for bs, total in ((17, 1700), (1, 40), (15, 15 * 20 + 7), (16, 16 * 20), (31, 31 * 12 + 30), (33, 33 * 12 + 1), (48, 48 * 9 + 47)):
        stream, plain = datagen.element_stream(total, bs, 7400 + bs, 1)
        t, b, offs = kc._offsets(stream)
        assert (t, b) == (total, bs)
        out.append(("small-bs%d" % bs, stream, plain, offs, total, bs))
    return out
