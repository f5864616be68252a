"""GPU tests (-m gpu) of the Snappy framing format (.sz) and CRC-32C through the C ABI and the binding: the case lists of
tests/test_sz_emulated.py on the device with guard bytes around every dst.  All comparisons are exact, against the Python
model of tests/sz_cases.py.  Everything is small: the largest item is a few hundred KiB."""
import numpy as np
import pytest

import datagen
import sz_cases as sz
from test_gpu_raw import GAP, Batch

pytestmark = pytest.mark.gpu
FILL = bytes([0xEE])


@pytest.fixture(scope="module")
def shb():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as binding
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return binding


@pytest.fixture(scope="module")
def intact():
    return sz.intact_streams()


@pytest.fixture(scope="module")
def damaged():
    return sz.damaged_streams()


def gpu_decompress(shb, items, max_chunks, flags=0):
    import torch
    b = Batch(items)
    b.d_bad = torch.full((b.n + 1,), 0x66, dtype=torch.int32, device="cuda")
    shb.sz_decompress_batch(shb.make_raw_items(b.entries), b.n, max_chunks, b.d_out_len, b.d_status, b.d_bad, b.d_result, flags=flags)
    b.fetch()
    b.bad = [int(x) & 0xffffffff for x in b.d_bad.cpu().numpy()]
    assert b.bad[b.n] == 0x66
    return b


def gpu_compress(shb, items, chunk_len, max_chunks):
    b = Batch(items)
    shb.sz_compress_batch(shb.make_raw_items(b.entries), b.n, chunk_len, max_chunks, b.d_out_len, b.d_status, b.d_result)
    b.fetch()
    return b


def check_decoded(b, i, s, capacity, verify=True):
    st, n, plain, bad = sz.read_sz(s, capacity, verify)
    assert (b.status[i], b.out_len[i], b.bad[i]) == (st, n, bad), (i, b.status[i], b.out_len[i], b.bad[i], st, n, bad)
    w = b.window(i)
    if st == sz.OK:
        assert w[:n] == plain and w[n:] == FILL * (capacity - n), i
    elif isinstance(plain, list):                      # a bad chunk: the others are decoded, nothing behind the total is touched
        at = 0
        for piece in plain:
            if piece is None:
                break
            assert w[at:at + len(piece)] == piece, i
            at += len(piece)
        assert w[n:] == FILL * (capacity - n), i
    else:
        assert w == FILL * capacity, i                 # a fault of the chain, or no room: not one byte written


def test_gpu_crc32c_every_length_at_every_alignment(shb):
    """The lengths of the emulator test at 16 start alignments and the six published vectors, one launch."""
    import torch
    r = datagen.random_bytes(65537 + 16, seed=31)
    datas = [d for d, _, _ in sz.CRC_VECTORS] + [r[k:k + n] for n in sz.crc_lengths() + list(range(250, 262)) + [16383, 16385] for k in range(16)]
    blob, at = bytearray(), []
    for k, d in enumerate(datas):
        blob += bytes(1 + k % 3)
        at.append(len(blob))
        blob += d
    d_src = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()
    d_crc = torch.full((len(datas) + 1,), 0x77, dtype=torch.int32, device="cuda")
    shb.crc32c_batch(shb.make_crc_items([(d_src.data_ptr() + a, len(d)) for a, d in zip(at, datas)]), len(datas), d_crc)
    torch.cuda.synchronize()
    got = [int(x) & 0xffffffff for x in d_crc.cpu().numpy()]
    assert got[-1] == 0x77
    want = [sz.crc32c(d) for d in datas]
    assert got[:-1] == want, [(k, len(datas[k])) for k in range(len(datas)) if got[k] != want[k]][:5]
    assert want[:6] == [c for _, c, _ in sz.CRC_VECTORS]


@pytest.mark.parametrize("chunk_len", [1, 17, 4096, 32768, 65535])
def test_gpu_sz_compress_is_the_model_writer_over_the_oracles_blocks(shb, chunk_len):
    mix = sz.text_random_mix(3 * 65536 + 2, 7)
    rnd = datagen.random_bytes(70000, seed=8)
    limit = 3000 if chunk_len < 100 else 300000
    sizes = [n for n in sorted({0, 1, chunk_len - 1, chunk_len, chunk_len + 1, 3 * chunk_len + 1, 65535, 65536}) if n <= limit]
    plains = [mix[5:5 + n] for n in sizes] + [rnd[:n] for n in sizes if n]
    if chunk_len >= 4096:
        plains += [mix, rnd, bytes(300000)]
    wants = [sz.write_sz_oracle(p, chunk_len) for p in plains]
    caps = [max(len(w) + (0, 7, -1)[k % 3], 0) for k, w in enumerate(wants)]
    chunks = sum(-(-len(p) // chunk_len) for p in plains)
    b = gpu_compress(shb, list(zip(plains, caps)), chunk_len, chunks)
    ok = 0
    for i, (p, w, cap) in enumerate(zip(plains, wants, caps)):
        assert shb.sz_compress_bound(len(p), chunk_len) == 10 + 8 * -(-len(p) // chunk_len) + len(p) >= len(w)
        if cap < len(w):
            assert (b.status[i], b.out_len[i]) == (sz.DST_TOO_SMALL, len(w)) and b.window(i) == FILL * cap, i
            continue
        ok += 1
        assert (b.status[i], b.out_len[i]) == (sz.OK, len(w)), (i, b.status[i], b.out_len[i], len(w))
        assert b.window(i) == w + FILL * (cap - len(w)), i
    assert b.result == [chunks, ok]
    # random bytes: every chunk of type 0x01, the bound exactly
    i = len(sizes) + len([n for n in sizes if n]) - 1
    if b.status[i] == sz.OK:
        assert b.out_len[i] == shb.sz_compress_bound(len(plains[i]), chunk_len)
    # and the device reads back what it wrote
    items = [(b.window(i)[:b.out_len[i]], len(p)) for i, p in enumerate(plains) if b.status[i] == sz.OK]
    d = gpu_decompress(shb, items, chunks)
    kept = [p for i, p in enumerate(plains) if b.status[i] == sz.OK]
    assert d.status[:d.n] == [sz.OK] * d.n and all(d.window(i) == p for i, p in enumerate(kept))


def test_gpu_sz_compress_max_chunks_and_bad_items(shb):
    chunk_len = 1000
    plains = [sz.text_random_mix(n, 9 + n) for n in (2500, 0, 3000, 1, 999)]
    wants = [sz.write_sz_oracle(p, chunk_len) for p in plains]
    items = [(p, len(w)) for p, w in zip(plains, wants)]
    b = gpu_compress(shb, items, chunk_len, 5)
    assert b.status[:5] == [sz.OK, sz.OK, sz.TOO_LARGE, sz.TOO_LARGE, sz.TOO_LARGE] and b.result == [8, 2]
    assert b.window(0) == wants[0] and b.window(1) == sz.IDENTIFIER and b.window(2) == FILL * len(wants[2])
    b = gpu_compress(shb, items, chunk_len, 0)
    assert b.status[:5] == [sz.TOO_LARGE, sz.OK, sz.TOO_LARGE, sz.TOO_LARGE, sz.TOO_LARGE] and b.result == [8, 1]
    b = gpu_compress(shb, [(b"", 0, 1, 10), (b"", 10, 1, 0), (b"abc", 64, 0, 1 << 32), (b"abcd" * 10, 5), (b"", 9), (b"x", 19, 2)], chunk_len, 4)
    assert b.status[:6] == [sz.INVALID, sz.OK, sz.TOO_LARGE, sz.DST_TOO_SMALL, sz.DST_TOO_SMALL, sz.DST_TOO_SMALL]
    assert b.window(1) == sz.IDENTIFIER and b.out_len[4] == 10 and b.out_len[5] == 19
    assert shb.sz_compress_bound(5, 0) == 0 and shb.sz_compress_scratch_bytes(65536, 1, 1) == 0
    with pytest.raises(shb.SnappyHipError):
        gpu_compress(shb, items, 65536, 8)


def test_gpu_sz_decode_intact_and_damaged_streams_in_one_batch(shb, intact, damaged):
    """pyarrow-made chunks of 65,536 bytes, skippable chunks, concatenated files, zero-length chunks and every damaged case, each
    at capacities exact, generous and one short, in one launch; each verdict is the model reader's."""
    items, streams = [], []
    for s in [x[0] for x in intact.values()] + list(damaged.values()):
        n = sz.read_sz(s)[1]
        for cap in (n, n + 3) + ((n - 1,) if n else ()):
            items.append((s, cap))
            streams.append(s)
    b = gpu_decompress(shb, items, 400)
    for i, (s, it) in enumerate(zip(streams, items)):
        check_decoded(b, i, s, it[1])
    assert b.result[1] == sum(st == sz.OK for st in b.status[:b.n]) > 0
    for name, (s, plain) in intact.items():
        k = streams.index(s)
        assert b.status[k] == sz.OK and b.window(k) == plain, name


def test_gpu_sz_decode_no_verify_sizing_and_limits(shb, intact, damaged):
    for name in ("crc_word_bit_chunk0", "crc_word_bit_chunk2", "two_bad_chunks", "elements_damaged", "payload_bit_uncompressed"):
        s = damaged[name]
        n = sz.read_sz(s)[1]
        b = gpu_decompress(shb, [(s, n)], 8, flags=sz.NO_VERIFY)
        check_decoded(b, 0, s, n, verify=False)
        assert (b.status[0] == sz.OK) == (name != "elements_damaged"), name
    s, plain = intact["pyarrow_65536"]
    n = len(plain)
    b = gpu_decompress(shb, [(s, 0, 2), (s, n, 2), (s, n, 1), (s, n, 0, 0x7ffff001)], 16)
    assert b.status[:4] == [sz.DST_TOO_SMALL, sz.DST_TOO_SMALL, sz.INVALID, sz.TOO_LARGE] and b.out_len[:4] == [n, n, 0, 0]
    assert all(b.window(i) == FILL * b.caps[i] for i in range(4)) and b.bad[:4] == [sz.NONE] * 4
    a, pa = intact["two_files"]
    items = [(a, len(pa)), (sz.IDENTIFIER, 0), (s, n), (a, len(pa))]
    b = gpu_decompress(shb, items, 5)
    assert b.status[:4] == [sz.OK, sz.OK, sz.TOO_LARGE, sz.TOO_LARGE] and b.result == [8, 2] and b.window(2) == FILL * n and b.out_len[2] == n
    b = gpu_decompress(shb, items, 8)
    assert b.status[:4] == [sz.OK] * 4 and b.result == [8, 4] and b.window(2) == plain
    b = gpu_decompress(shb, items, 0)
    assert b.status[:4] == [sz.TOO_LARGE, sz.OK, sz.TOO_LARGE, sz.TOO_LARGE] and b.result == [8, 1]
    with pytest.raises(shb.SnappyHipError):
        gpu_decompress(shb, items, 8, flags=2)


def test_gpu_sz_drop_in_pair_round_trip_and_verdicts(shb, intact, damaged):
    plain = sz.text_random_mix(150000, 11)
    st, stream, _ = shb.sz_compress_host(plain, 32768)
    assert st == 0 and stream == sz.write_sz_oracle(plain, 32768)
    st, got, _ = shb.sz_decompress_host(stream)
    assert st == 0 and got == plain
    st, stream, _ = shb.sz_compress_host(b"", 4096)
    assert st == 0 and stream == sz.IDENTIFIER and shb.sz_decompress_host(stream)[:2] == (0, b"")
    s, p = intact["pyarrow_65536"]
    assert shb.sz_decompress_host(s)[:2] == (0, p)
    for name in ("crc_word_bit_chunk2", "reserved_unskippable_02", "truncated_by_1", "varint_disagrees_longer", "identifier_missing"):
        st, got, _ = shb.sz_decompress_host(damaged[name])
        assert st != 0 and got == b"", name
    assert shb.sz_decompress_host(damaged["crc_word_bit_chunk2"], flags=sz.NO_VERIFY)[0] == 0
