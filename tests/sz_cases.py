"""A Python model of the Snappy framing format (.sz), written from the format's description in include/snappy_hip.h, and the
vectors the emulator, GPU and CLI tests of the .sz codec share: a bitwise CRC-32C (and a table walk checked against it), the
mask, a frame writer and a strict reader whose verdicts are the ones snappy_hip_sz_decompress_batch documents.

No .sz producer exists where these tests were written (no python-snappy, no cramjam, no snzip), so third-party CONTENT comes
from pyarrow.Codec('snappy') -- Google's Snappy -- compressing each chunk, which the model then frames; that includes chunks
of 65,536 bytes, which this project's compressor never writes."""
import os
import sys

import datagen
import raw_cases as rc

OK, INVALID, DST_TOO_SMALL, TOO_LARGE, CRC_MISMATCH, UNSUPPORTED = 0, 1, 5, 6, 7, 8
NO_VERIFY = 1
NONE = 0xffffffff
IDENTIFIER = b"\xff\x06\x00\x00sNaPpY"
MAX_CHUNK = 65536
POLY = 0x82F63B78

# (input, CRC-32C, masked)
CRC_VECTORS = [(b"123456789", 0xE3069283, 0xC78AB0E5), (bytes(32), 0x8A9136AA, 0x0FD7FFFA), (b"\xff" * 32, 0x62A8AB43, 0xF909B029),
               (bytes(range(32)), 0x46DD794E, 0x951F7892), (bytes(range(31, -1, -1)), 0x113FDB5C, 0x593B0D57), (b"", 0, 0xA282EAD8)]


def crc32c_bitwise(data, crc=0):
    c = crc ^ 0xffffffff
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
    return c ^ 0xffffffff


def _make_table():
    t = []
    for b in range(256):
        c = b
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
        t.append(c)
    return t


_TABLE = _make_table()


def crc32c(data):
    """the bitwise CRC's value by a byte table made with the bitwise step (tests/test_sz_model.py holds the two together)"""
    c = 0xffffffff
    t = _TABLE
    for b in data:
        c = (c >> 8) ^ t[(c ^ b) & 0xff]
    return c ^ 0xffffffff


def mask(c):
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xffffffff


def gf_mul(a, b):
    """a * b mod P, bit 31 = x^0 (csrc/snappy_crc32c.hpp gf_mul)"""
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


# ---- the frame writer ----
def chunk(kind, body):
    assert len(body) < 1 << 24
    return bytes([kind]) + len(body).to_bytes(3, "little") + body


def data_chunk(plain, raw=None, crc=None):
    """type 0x00 carrying the raw stream `raw`, or type 0x01 carrying `plain` (raw is None); crc: the word to store"""
    word = (mask(crc32c(plain)) if crc is None else crc).to_bytes(4, "little")
    return chunk(0x00, word + raw) if raw is not None else chunk(0x01, word + plain)


def write_sz(plain, chunk_len, compress):
    """The identifier, then one chunk per chunk_len bytes; compress(piece) -> a raw Snappy stream, used iff it is shorter than
    the piece (what snappy_hip_sz_compress_batch documents)."""
    out = bytearray(IDENTIFIER)
    for at in range(0, len(plain), chunk_len):
        piece = plain[at:at + chunk_len]
        raw = compress(piece)
        out += data_chunk(piece, raw if len(raw) < len(piece) else None)
    return bytes(out)


def oracle_raw(piece, block_size=None):
    """varint32(n) + the elements the reference's compressor writes for `piece` as one block of a stream of block_size blocks
    (the hash table is sized by the block size, not by the piece)"""
    import oracle_lib as oracle
    block_size = block_size or min(max(len(piece), 1), 65535)
    assert len(piece) <= block_size
    return rc.trs.convert(oracle.compress(piece, block_size))


def write_sz_oracle(plain, chunk_len):
    return write_sz(plain, chunk_len, lambda piece: oracle_raw(piece, chunk_len))


def write_sz_pyarrow(plain, chunk_len):
    """Google's Snappy inside the model's frames; every chunk compressed, whatever it gains (a writer may)"""
    import pyarrow as pa
    codec = pa.Codec("snappy")
    out = bytearray(IDENTIFIER)
    for at in range(0, len(plain), chunk_len):
        piece = plain[at:at + chunk_len]
        out += data_chunk(piece, codec.compress(piece, asbytes=True))
    return bytes(out)


# ---- the strict reader ----
def read_sz(s, capacity=None, verify=True):
    """-> (status, out_len, plaintext or None, bad_chunk): what snappy_hip_sz_decompress_batch answers for one item with
    `capacity` bytes at dst (None: room for everything).  With a bad chunk the plaintext holds None in that chunk's place:
    (status, out_len, [pieces], bad_chunk)."""
    if len(s) > rc.RAW_MAX_LEN:
        return TOO_LARGE, 0, None, NONE
    at, identified, chunks = 0, False, []          # chunks: (kind, crc word, body, uncompressed length)
    while at < len(s):
        if at + 4 > len(s):
            return INVALID, 0, None, NONE
        kind, L = s[at], int.from_bytes(s[at + 1:at + 4], "little")
        if at + 4 + L > len(s):
            return INVALID, 0, None, NONE
        body = s[at + 4:at + 4 + L]
        if kind == 0xff:
            if body != b"sNaPpY":
                return INVALID, 0, None, NONE
            identified = True
        elif not identified:
            return INVALID, 0, None, NONE
        elif kind <= 1:
            if L < 4:
                return INVALID, 0, None, NONE
            n = L - 4
            if kind == 0:
                h = rc.header_parses(body[4:])
                if h is None:
                    return INVALID, 0, None, NONE
                n = h[0]
            if n > MAX_CHUNK:
                return INVALID, 0, None, NONE
            chunks.append((kind, int.from_bytes(body[:4], "little"), body[4:], n))
        elif kind < 0x80:
            return UNSUPPORTED, 0, None, NONE
        at += 4 + L
    if not identified:
        return INVALID, 0, None, NONE
    total = sum(c[3] for c in chunks)
    if total > rc.RAW_MAX_LEN:
        return TOO_LARGE, total, None, NONE
    if capacity is not None and total > capacity:
        return DST_TOO_SMALL, total, None, NONE
    pieces, status, bad = [], OK, NONE
    for k, (kind, word, body, n) in enumerate(chunks):
        st, piece = OK, body
        if kind == 0:
            st, _, piece = rc.expect(body, None)
        if st == OK and verify and mask(crc32c(piece)) != word:
            st = CRC_MISMATCH
        if st != OK and status == OK:
            status, bad = st, k
        pieces.append(piece if st in (OK, CRC_MISMATCH) else None)
    if status == OK:
        return OK, total, b"".join(pieces), NONE
    return status, total, pieces, bad


# ---- plaintexts and streams ----
def text_random_mix(n, seed):
    """stretches of text and of random bytes in turn: chunks of both types in one stream"""
    with open(os.path.join(rc.HERE, "golden", "terror2.txt"), "rb") as f:
        return datagen.text_random_interleave(f.read(), n, seed=seed, chunk=9000)


def intact_streams():
    """name -> (stream, plaintext): what a reader must accept"""
    v = {}
    text = text_random_mix(200000, 5)
    v["pyarrow_65536"] = (write_sz_pyarrow(text, 65536), text)
    v["pyarrow_tail_1"] = (write_sz_pyarrow(text[:65537], 65536), text[:65537])
    zeros = bytes(140000)
    v["pyarrow_zeros"] = (write_sz_pyarrow(zeros, 65536), zeros)
    rnd = datagen.random_bytes(70000, seed=9)
    v["plain_65536"] = (IDENTIFIER + data_chunk(rnd[:65536]) + data_chunk(rnd[65536:]), rnd)
    a, b = text[:3000], text[3000:7001]
    ra, rb = oracle_raw(a), oracle_raw(b)
    v["padding_and_skippable"] = (IDENTIFIER + chunk(0xfe, bytes(13)) + data_chunk(a, ra) + chunk(0x80, b"anything") + chunk(0xfd, b"") +
                                  data_chunk(b, rb) + chunk(0xfe, b""), a + b)
    v["two_files"] = (IDENTIFIER + data_chunk(a, ra) + IDENTIFIER + data_chunk(b), a + b)
    v["zero_length_chunks"] = (IDENTIFIER + data_chunk(b"") + data_chunk(a, ra) + data_chunk(b"", b"\x00") + data_chunk(b, rb) + data_chunk(b""), a + b)
    v["identifier_alone"] = (IDENTIFIER, b"")
    v["padded_varint"] = (IDENTIFIER + data_chunk(a[:100], bytes([0x80 | 100, 0x80, 0x00]) + rc.literal(a[:100])), a[:100])
    return v


def damaged_streams():
    """name -> stream; the expected verdict of each is read_sz's"""
    v = {}
    text = text_random_mix(30000, 6)
    a, b, c = text[:9000], text[9000:20000], text[20000:]
    ca, cb, cc = data_chunk(a, oracle_raw(a)), data_chunk(b), data_chunk(c, oracle_raw(c))
    good = IDENTIFIER + ca + cb + cc

    def flip(s, at, bit=0):
        return s[:at] + bytes([s[at] ^ (1 << bit)]) + s[at + 1:]

    v["crc_word_bit_chunk0"] = flip(good, 10 + 4, 3)
    v["crc_word_bit_chunk2"] = flip(good, 10 + len(ca) + len(cb) + 7, 7)
    v["payload_bit_compressed"] = flip(good, 10 + 8 + 40, 2)                       # a literal's byte, most likely: decodes, CRC fails
    v["payload_bit_uncompressed"] = flip(good, 10 + len(ca) + 8 + 5000, 5)
    v["two_bad_chunks"] = flip(flip(good, 10 + len(ca) + 8 + 1, 0), 10 + 5, 0)    # the lowest-numbered one is named
    v["reserved_unskippable_02"] = IDENTIFIER + ca + chunk(0x02, b"what") + cb
    v["reserved_unskippable_7f"] = IDENTIFIER + chunk(0x7f, b"")
    v["identifier_missing"] = ca + cb
    v["identifier_wrong"] = b"\xff\x06\x00\x00sNaPpy" + ca
    v["identifier_wrong_length"] = b"\xff\x07\x00\x00sNaPpY\x00" + ca
    v["identifier_not_first"] = chunk(0xfe, b"") + IDENTIFIER + ca
    v["identifier_wrong_later"] = IDENTIFIER + ca + b"\xff\x06\x00\x00SNaPpY" + cb
    v["no_identifier_at_all"] = b""
    v["truncated_by_1"] = good[:-1]
    v["truncated_in_a_header"] = IDENTIFIER + ca + cb[:3]
    v["data_chunk_L_3"] = IDENTIFIER + chunk(0x01, b"abc") + ca
    v["data_chunk_L_0_compressed"] = IDENTIFIER + chunk(0x00, b"")
    v["compressed_chunk_without_varint"] = IDENTIFIER + chunk(0x00, mask(0).to_bytes(4, "little"))
    big = datagen.random_bytes(65537, seed=3)
    v["uncompressed_65537"] = IDENTIFIER + data_chunk(big)
    v["varint_says_65537"] = IDENTIFIER + data_chunk(big, rc.varint(65537) + rc.literal(big))
    v["varint_disagrees_longer"] = IDENTIFIER + ca + data_chunk(b[:500], rc.varint(501) + rc.literal(b[:500])) + cc
    v["varint_disagrees_shorter"] = IDENTIFIER + data_chunk(b[:500], rc.varint(499) + rc.literal(b[:500])) + cc
    v["zero_varint_with_elements"] = IDENTIFIER + data_chunk(b"", b"\x00" + rc.literal(b"x")) + ca
    v["elements_damaged"] = IDENTIFIER + ca + data_chunk(b[:500], rc.varint(500) + rc.literal(b[:400]) + rc.copy2(64, 5000) + rc.literal(b[:36]))
    return v


def crc_lengths():
    return [0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 65535, 65536, 65537]


if __name__ == "__main__":          # python tests/sz_cases.py read FILE: the model reader's verdict and plaintext length
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    with open(sys.argv[2], "rb") as f:
        st, n, plain, bad = read_sz(f.read())
    print(st, n, bad)
