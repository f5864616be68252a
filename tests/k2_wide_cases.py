"""Cases for the wide block decoder (csrc/snappy_k2_wide.hpp; tests/test_k2_wide_emulated.py on the wave emulator,
tests/test_gpu_k2_wide.py on the GPU).  Test infrastructure only: plain Python + the oracle.

A job is k2_window_cases' (name, stream, at, out_len): the block whose u32 size word is at stream[at], decoded alone into
out_len bytes.  The yardsticks are K2 itself on the same job (status, and bytes where the status is OK) and the oracle
(k2_window_cases.check_job); the result words follow from K2's status and the limits alone (expected_result)."""
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
