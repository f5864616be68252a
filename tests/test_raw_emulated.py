"""CPU tests of the raw Snappy batch interface: the UNMODIFIED kernels of pim-compression_amd/csrc/snappy_raw.hpp (K2's decoder
in its raw form, K1's LDS-table form) on the lockstep wave emulator.  Every dst is a window of exactly its capacity between
inaccessible pages and every src ends at one, so one byte written outside a window or read behind a stream is a fault -- a
legitimate failure here, which is why every body below runs in a child process that names the step it is on.  All
comparisons are exact: decode against tools/to_raw_snappy.decode_raw, compress against convert(oracle.compress(...))."""
import os
import subprocess
import sys

import pytest

import datagen
import emu_raw_lib as er
import oracle_lib as oracle
import raw_cases as rc
from conftest import golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = bytes([rc.GUARD])


def step(*what):
    print("step", *what, flush=True)


def check_decoded(b, i, s, capacity):
    """item i of a finished batch against the format's CPU statement"""
    st, n, plain = rc.expect(s, capacity)
    assert int(b.status[i]) == st, (int(b.status[i]), st)
    assert int(b.out_len[i]) == n, (int(b.out_len[i]), n)
    w = b.window(i)
    if st == rc.OK:
        assert w[:n] == plain, next(k for k in range(n) if w[k] != plain[k])
        assert w[n:] == FILL * (capacity - n)
    elif st != rc.INVALID or n == 0:
        assert w == FILL * capacity                  # TOO_SMALL, TOO_LARGE, a bad header: not one byte written


def decode_alone(name, s, capacity=None, flags=0):
    step("decode", name)
    h = rc.header_parses(s)
    cap = capacity if capacity is not None else (h[0] if h and h[0] <= (1 << 22) else 0)
    rc_, b = er.decompress([(s, cap, flags)], grid=1)
    assert rc_ == 0, "a kernel wrote in front of a window"
    if flags & 2:
        cap_seen = 0
    else:
        cap_seen = cap
    st, n, plain = rc.expect(s, cap_seen)
    assert (int(b.status[0]), int(b.out_len[0])) == (st, n), (name, int(b.status[0]), int(b.out_len[0]), st, n)
    if not flags & 2:
        check_decoded(b, 0, s, cap)
    assert int(b.status[1]) == 0x55 and int(b.out_len[1]) == 0x5A5A5A5A5A5A5A5A      # nothing behind the arrays' last entry
    return b


# ---- decode ----
def body_fixtures():
    for name in rc.FIXTURES:
        s = rc.fixture_stream(name)
        b = decode_alone(name, s)
        assert int(b.status[0]) == rc.OK and b.window(0) == rc.fixture_plain(name)


def body_intact_vectors():
    for name, s in rc.intact_vectors().items():
        b = decode_alone(name, s)
        assert int(b.status[0]) == rc.OK, name


def body_damaged_vectors():
    for name, s in rc.damaged_vectors().items():
        h = rc.header_parses(s)
        b = decode_alone(name, s, capacity=h[0] if h else 64)
        assert int(b.status[0]) == rc.INVALID, name
        # and with room to spare: still nothing outside [dst, dst + length)
        step("decode", name, "with spare capacity")
        n = h[0] if h else 0
        r, b = er.decompress([(s, n + 4096)], grid=1)
        assert r == 0 and int(b.status[0]) == rc.INVALID and b.window(0)[n:] == FILL * 4096, name


def body_capacity():
    s = rc.intact_vectors()["all_types"]
    n = rc.header_parses(s)[0]
    assert int(decode_alone("exact", s, n).status[0]) == rc.OK
    assert int(decode_alone("one less", s, n - 1).status[0]) == rc.DST_TOO_SMALL
    b = decode_alone("sizing call", s, 0, flags=2)
    assert (int(b.status[0]), int(b.out_len[0])) == (rc.DST_TOO_SMALL, n)
    b = decode_alone("null dst with capacity", s, n, flags=2)        # a null dst counts as capacity 0
    assert int(b.status[0]) == rc.DST_TOO_SMALL and b.window(0) == FILL * n
    step("null src")
    r, b = er.decompress([(s, n, 1)], grid=1)
    assert (r, int(b.status[0]), int(b.out_len[0])) == (0, rc.INVALID, 0) and b.window(0) == FILL * n
    # lengths beyond SNAPPY_HIP_RAW_MAX_LEN: the header's, and src_len (the stream itself is never read that far)
    assert er.lib().emu_raw_max_len() == rc.RAW_MAX_LEN >= 1 << 30 and er.lib().emu_raw_dst_fill() == rc.GUARD
    big = rc.varint(rc.RAW_MAX_LEN + 1) + rc.literal(b"x")
    b = decode_alone("header beyond the maximum", big, 16)
    assert (int(b.status[0]), int(b.out_len[0])) == (rc.TOO_LARGE, rc.RAW_MAX_LEN + 1)
    step("src_len beyond the maximum")
    r, b = er.decompress([(s, n, 0, rc.RAW_MAX_LEN + 1)], grid=1)
    assert (r, int(b.status[0]), int(b.out_len[0])) == (0, rc.TOO_LARGE, n) and b.window(0) == FILL * n
    step("the largest header that is not too large, no room")
    r, b = er.decompress([(rc.varint(rc.RAW_MAX_LEN) + rc.literal(b"x"), 5)], grid=1)
    assert (r, int(b.status[0]), int(b.out_len[0])) == (0, rc.DST_TOO_SMALL, rc.RAW_MAX_LEN)
    step("no items")
    r, b = er.decompress([], grid=1)
    assert r == 0


def body_mixed_batch():
    """intact, damaged, too small and fixture items in ONE launch of two wavefronts"""
    items, streams = [], []
    for s in list(rc.intact_vectors().values()) + list(rc.damaged_vectors().values()) + [rc.fixture_stream("coding"), rc.fixture_stream("alice")]:
        h = rc.header_parses(s)
        n = h[0] if h else 0
        for cap in (n, n + 3) + ((n - 1,) if n else ()):
            items.append((s, cap))
            streams.append(s)
    step("mixed batch of", len(items))
    r, b = er.decompress(items, grid=2)
    assert r == 0
    for i, (s, cap) in enumerate(items):
        step("item", i)
        check_decoded(b, i, s, cap)
    assert sorted(set(int(x) for x in b.status[:len(items)])) == [rc.OK, rc.INVALID, rc.DST_TOO_SMALL]


def body_k2_window_vectors():
    """tests/k2_window_cases.py's hand-made blocks as raw streams: a block's payload behind the header of its output length is a
    raw stream; the raw decoder must agree with the format's CPU statement on each (literals above 64 KiB included)."""
    import k2_window_cases as kc
    for k, (name, stream, at, out_len) in enumerate(kc.hand_jobs()):
        size = int.from_bytes(stream[at:at + 4], "little")
        if at + 4 + size > len(stream):
            continue
        if out_len == 65535 and k % 8:               # (a second each on the emulator, a hundred of them: every eighth)
            continue
        decode_alone(name, rc.varint(out_len) + stream[at + 4:at + 4 + size])


def body_damaged_rich_streams():
    """600 mutations of streams no greedy compressor writes: the decoder, the check and the split call against the format's CPU
    statement, which shares no code with any of them"""
    import emu_check_lib as ec
    import emu_raw_split_lib as es
    import raw_split_cases as sc
    items = sc.damaged_rich_streams()
    want = [rc.expect(s, n) for s, n in items]
    verdicts = [w[0] for w in want]
    print("expect's verdicts", verdicts.count(rc.OK), verdicts.count(rc.INVALID), flush=True)
    assert len(items) == 600 and verdicts.count(rc.OK) >= 100 and verdicts.count(rc.INVALID) >= 100 and set(verdicts) == {rc.OK, rc.INVALID}
    step("decode", len(items))
    r, b = er.decompress(items, grid=3)
    assert r == 0
    for i, (s, n) in enumerate(items):
        step("item", i)
        check_decoded(b, i, s, n)
    step("check")
    assert ec.raw_check([s for s, _ in items], grid=3) == [w[:2] for w in want]
    step("split")
    r, sp = es.decompress_split(items, 256, 128, grid=3)
    assert r == 0
    for i, (s, n) in enumerate(items):
        step("split item", i)
        check_decoded(sp, i, s, n)
    res = [int(x) for x in sp.result[:4]]
    assert res[0] > 0 and res[2] >= verdicts.count(rc.INVALID) and sum(res) == len(items), res


# ---- compress ----
def want_raw(plain, bs):
    return rc.trs.convert(oracle.compress(plain, bs))


def check_compressed(b, i, plain, bs, capacity):
    want = want_raw(plain, bs)
    w = b.window(i)
    if len(want) <= capacity:
        assert (int(b.status[i]), int(b.out_len[i])) == (rc.OK, len(want)), (i, int(b.status[i]), int(b.out_len[i]), len(want))
        assert w[:len(want)] == want, next(k for k in range(len(want)) if w[k] != want[k])
        assert w[len(want):] == FILL * (capacity - len(want))
    else:
        assert (int(b.status[i]), int(b.out_len[i])) == (rc.DST_TOO_SMALL, len(want))
        assert w == FILL * capacity
    return len(want) <= capacity


def plain_for(n, seed):
    text = golden_bytes("plrabn12.txt")
    kinds = (lambda: text[seed * 1000:seed * 1000 + n], lambda: datagen.lz_structured(n, seed), lambda: datagen.random_bytes(n, seed),
             lambda: datagen.zeros(n), lambda: datagen.low_entropy(n, seed=seed))
    return kinds[seed % len(kinds)]()


def body_compress(bs, form):
    plains = [plain_for(n, k + bs % 7) for k, n in enumerate(rc.compress_lengths(bs))]
    wants = [want_raw(p, bs) for p in plains]
    frags = sum((len(p) + bs - 1) // bs for p in plains)
    # capacities: exact, one short (items 2 and 5), generous
    caps = [len(w) - 1 if i in (2, 5) else (len(w) if i % 2 else len(w) + 9) for i, w in enumerate(wants)]
    step("compress", bs, form, "fragments", frags)
    r, b = er.compress(list(zip(plains, caps)), bs, frags, grid=3, form=form)
    assert r == 0
    ok = sum(check_compressed(b, i, p, bs, caps[i]) for i, p in enumerate(plains))
    assert [int(x) for x in b.result] == [frags, ok] and ok == len(plains) - 2
    # the new decoder reads what it wrote
    step("round trip", bs, form)
    r, d = er.decompress([(w, len(p)) for w, p in zip(wants, plains)], grid=2)
    assert r == 0
    for i, p in enumerate(plains):
        assert int(d.status[i]) == rc.OK and d.window(i) == p, i


def body_compress_max_fragments():
    bs = 1000
    plains = [plain_for(n, k) for k, n in enumerate((2500, 0, 999, 3001, 0, 1, 700))]
    need = sum((len(p) + bs - 1) // bs for p in plains)                 # 3 + 0 + 1 + 4 + 0 + 1 + 1
    caps = [len(want_raw(p, bs)) for p in plains]
    for max_fragments in (need, need - 1, 7, 4, 3, 0):
        step("max_fragments", max_fragments)
        r, b = er.compress(list(zip(plains, caps)), bs, max_fragments, grid=2)
        assert r == 0
        ok = 0
        first = 0
        for i, p in enumerate(plains):
            n = (len(p) + bs - 1) // bs
            if n and first + n > max_fragments:
                assert (int(b.status[i]), int(b.out_len[i])) == (rc.TOO_LARGE, 0) and b.window(i) == FILL * caps[i], i
            else:
                ok += check_compressed(b, i, p, bs, caps[i])
            first += n
        assert [int(x) for x in b.result] == [need, ok], ([int(x) for x in b.result], need, ok)
    step("bad items")
    r, b = er.compress([(b"abc", 16, 1), (b"", 1, 1, 0), (b"abc", 16, 0, 1 << 32), (b"abcd" * 10, 0, 2)], bs, 8, grid=1)
    assert r == 0
    assert [int(x) for x in b.status[:4]] == [rc.INVALID, rc.OK, rc.TOO_LARGE, rc.DST_TOO_SMALL]
    assert b.window(1) == b"\x00" and int(b.out_len[1]) == 1 and int(b.out_len[3]) == len(want_raw(b"abcd" * 10, bs))
    assert [int(x) for x in b.result] == [1, 1]


def body_compress_goldens():
    for name in ("alice", "coding", "terror2"):
        plain = golden_bytes(name + ".txt")
        want = rc.trs.convert(golden_bytes(name + ".snappy"))
        assert want == want_raw(plain, 32768)
        step("golden", name)
        r, b = er.compress([(plain, len(want))], 32768, 8, grid=2)
        assert r == 0 and int(b.status[0]) == rc.OK and b.window(0) == want, name


BODIES = {f.__name__[5:]: f for f in (body_fixtures, body_intact_vectors, body_damaged_vectors, body_capacity, body_mixed_batch,
                                      body_k2_window_vectors, body_damaged_rich_streams, body_compress, body_compress_max_fragments, body_compress_goldens)}


def in_child(name, *args):
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import conftest, test_raw_emulated as t\n"
            "t.BODIES[sys.argv[2]](*[int(a) for a in sys.argv[3:]])\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code, HERE, name] + [str(a) for a in args], capture_output=True, text=True, timeout=1500)
    lines = out.stdout.strip().splitlines()
    last = next((ln for ln in reversed(lines) if ln.startswith("step ")), "none")
    assert out.returncode == 0 and lines and lines[-1] == "ok", \
        ("status %d (negative: a signal, i.e. an access outside a guarded buffer) at %s" % (out.returncode, last), out.stderr[-2000:])


def test_decode_third_party_fixtures():
    """Streams of Apache Arrow's Snappy codec (Google's Snappy): references across 32 KiB boundaries with offsets up to 64,926
    (plrabn12), literals of 65,536 bytes (random bytes), 300,000 zero bytes."""
    in_child("fixtures")


def test_decode_intact_vectors():
    """Literals of 65,537 and 300,000 bytes (a block decoder's 64 KiB literal bound would refuse them), COPY_4 offsets above
    65,535, COPY_2 of 65,535, overlapping copies across a 64 KiB boundary, empty, one byte, headers of 1..5 bytes."""
    in_child("intact_vectors")


def test_decode_damaged_vectors():
    in_child("damaged_vectors")


def test_decode_capacity_and_limits():
    in_child("capacity")


def test_decode_mixed_batch_with_fewer_wavefronts_than_items():
    in_child("mixed_batch")


def test_decode_k2_window_vectors_as_raw_streams():
    in_child("k2_window_vectors")


def test_decode_check_and_split_of_damaged_rich_streams_against_the_independent_decoder():
    """(status, out_len) of snappy_hip_raw_decompress_batch, _raw_check_batch and _raw_decompress_split_batch equal
    raw_cases.expect on every one of 600 mutated streams, and accepted bytes are decode_raw's."""
    in_child("damaged_rich_streams")


@pytest.mark.parametrize("form", [3, 2])
@pytest.mark.parametrize("bs", [64, 1000, 32768, 65535])
def test_compress_items_around_a_fragment(bs, form):
    """Items of 0, 1, 63, 64, block_size - 1, block_size, block_size + 1 and several fragments in one batch, both forms of
    K1's parse: byte for byte convert(oracle.compress(...)); capacity exact and one short; then decoded by the new decoder."""
    in_child("compress", bs, form)


def test_compress_max_fragments_and_bad_items():
    in_child("compress_max_fragments")


def test_compress_goldens_equal_the_converted_reference_streams():
    in_child("compress_goldens")


def test_compressed_items_are_read_by_pyarrow():
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("snappy")
    plains = [plain_for(n, k) for k, n in enumerate((0, 1, 70, 5000, 40000))]
    caps = [len(want_raw(p, 4096)) for p in plains]
    r, b = er.compress(list(zip(plains, caps)), 4096, 16, grid=2)
    assert r == 0
    for i, p in enumerate(plains):
        assert int(b.status[i]) == rc.OK
        assert codec.decompress(b.window(i), decompressed_size=len(p), asbytes=True) == p


def test_fixtures_match_their_record():
    for name in rc.FIXTURES:
        assert rc.trs.decode_raw(rc.fixture_stream(name)) == rc.fixture_plain(name)
