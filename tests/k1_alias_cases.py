"""Inputs of the alias tests (tests/test_k1_alias_emulated.py, tests/test_gpu_k1_alias.py): windows built so that lanes of
K1's stream form share a slot of the duplicate analysis (csrc/snappy_k1_stream.hpp: stream_analyse) with earlier lanes of
another hash -- aliases -- in both of its tables.  Every input is compared with the oracle byte for byte.

The hash of a 4-byte gram is (le32 * 0x1e35a7bd) >> shift; the multiplier is odd, so a gram exists for any wanted product.
The analysis indexes one table by the hash's bits 0.. and the other by its bits 5.., 8 bits each in the global-table kernels
(256 slots), 9 in the LDS-table kernel (512).  For a lane of hash H, a lane of hash H ^ (1 << abit) is an alias in the first
table when abit is above the index (abit = the hash's top bit: both sizes; abit = 8: 256 slots only), and a lane of hash
H ^ 1 is one in the second.

An input is ONE block: a dictionary of sixteen 8-byte chunks, then one region per case.  A region starts with the strings the
case copies from, each behind a chunk (a copy: the scan is at stride 1 behind it, so the string's first grams are inserted),
then a window of eight chunks (eight copies: the stream form is running), then the case's window, filled up with chunks."""
import functools

import numpy as np

MUL = 0x1e35a7bd
MUL_INV = pow(MUL, -1, 1 << 32)
BLOCKS = (32768, 4097)


def hash_bits(n):
    """bits of the hash in a block of n bytes (snappy_kernels.hpp: table_entries_for)"""
    ts = 256
    while ts < 16384 and ts < n:
        ts <<= 1
    return ts.bit_length() - 1


def hash_of(gram, bits):
    return ((int.from_bytes(gram, "little") * MUL) & 0xffffffff) >> (32 - bits)


def gram_for(h, bits, low):
    """the 4 bytes whose hash is h; `low` (any number) picks one of the 2^(32 - bits) of them"""
    shift = 32 - bits
    prod = (h << shift) | (low % (1 << shift))
    g = ((prod * MUL_INV) & 0xffffffff).to_bytes(4, "little")
    assert hash_of(g, bits) == h
    return g


@functools.lru_cache(maxsize=None)
def overlapping(bits, s, seed):
    """s + 4 bytes in which lane s (1 or 2) has an alias in front of it in both tables of 256 AND of 512 slots and no lane of
    its own hash: found by search, since the grams of adjacent lanes overlap.  s = 1 needs ONE lane that is an alias in both
    tables: a hash that differs above both indexes -- bit 13 of 14 for 256 slots, impossible for 512 (None where there is none)."""
    if s == 1 and bits < 14:
        return None
    r = np.random.default_rng(seed)
    lo9, hi9 = 0x1ff, 0x1ff << 5
    for _ in range(64):
        b = r.integers(0, 256, size=(1 << 21, s + 4), dtype=np.uint64)
        h = [(((b[:, i] | (b[:, i + 1] << 8) | (b[:, i + 2] << 16) | (b[:, i + 3] << 24)) * MUL) & 0xffffffff) >> (32 - bits) for i in range(s + 1)]
        if s == 1:                      # 256 slots: index bits 0-7 and 5-12
            ok = (h[0] ^ h[1]) == (1 << 13)
        else:
            ok = (((h[0] ^ h[2]) & lo9) == 0) & (((h[1] ^ h[2]) & hi9) == 0) & (h[0] != h[2]) & (h[1] != h[2])
        idx = np.flatnonzero(ok)
        if idx.size:
            return bytes(int(v) for v in b[idx[0]])
    raise AssertionError("no overlapping grams found")


class _Block:
    def __init__(self, n, abit, seed):
        self.n, self.bits = n, hash_bits(n)
        self.abit = self.bits - 1 if abit == "top" else abit
        self.r = np.random.default_rng(seed)
        self.buf = bytearray()
        self.dic = [self.fresh_bytes(8) for _ in range(16)]
        for c in self.dic:
            self.buf += c
        self.used = set()

    def fresh_bytes(self, k):
        return self.r.integers(0, 256, size=k, dtype=np.uint8).tobytes()

    def fresh(self, k=4):
        self.buf += self.fresh_bytes(k)

    def chunk(self):
        self.buf += self.dic[int(self.r.integers(0, 16))]

    def put(self, b):
        self.buf += b

    def to_lane(self, lane):
        """fill with chunks (and fewer than 8 fresh bytes) up to the next position at `lane` of a window"""
        k = (lane - len(self.buf)) % 64
        self.fresh(k % 8)
        for _ in range(k // 8):
            self.chunk()

    def lead(self, lane=0):
        """a window of eight copies in front of the case's window, which starts at `lane`"""
        self.to_lane(lane)
        for _ in range(8):
            self.chunk()

    def planted(self, b):
        """`b` where the case's window can copy it from: behind a chunk, with two chunks behind it"""
        self.chunk()
        self.put(b)
        self.chunk()
        self.chunk()

    def hashes(self):
        """(H, gram of H's alias in the first table, gram of its alias in the second), H not used in this block before"""
        while True:
            h = int(self.r.integers(2, 1 << self.bits))
            trio = {h, h ^ (1 << self.abit), h ^ 1}
            if not (trio & self.used):
                self.used |= trio
                return h, self.gram(h ^ (1 << self.abit)), self.gram(h ^ 1)

    def gram(self, h):
        return gram_for(h, self.bits, int(self.r.integers(0, 1 << 30)))


def _build(n, abit, seed):
    k = _Block(n, abit, seed)

    # (a) aliased in both tables by two earlier lanes, no earlier lane of its own hash: a miss, and a hit on a planted gram
    h, p1, p2 = k.hashes()
    k.lead()
    k.chunk(), k.put(p1), k.put(p2), k.put(k.gram(h)), k.fresh(), k.chunk()
    h, p1, p2 = k.hashes()
    u = k.gram(h) + k.fresh_bytes(4)
    k.planted(u)
    k.lead()
    k.chunk(), k.put(p1), k.put(p2), k.put(u), k.fresh(), k.chunk()

    # (b) a true partner hidden behind the aliases.  Probed (a miss, inserted): the lane hits it, 12 bytes back.
    h, p1, p2 = k.hashes()
    q = k.gram(h)
    k.lead()
    k.chunk(), k.put(q), k.put(p1), k.put(p2), k.put(q), k.fresh(), k.chunk()
    # ... the same with another gram of the same hash: a miss on the partner
    h, p1, p2 = k.hashes()
    k.lead()
    k.chunk(), k.put(k.gram(h)), k.put(p1), k.put(p2), k.put(k.gram(h)), k.fresh(), k.chunk()
    # ... inside a copy (not inserted): the lane hits the planted gram far back, not the partner
    h, p1, p2 = k.hashes()
    q = k.gram(h)
    u = k.fresh_bytes(4) + q
    k.planted(u)
    k.lead()
    k.fresh(), k.put(u), k.put(p1), k.put(p2), k.put(q), k.fresh(), k.chunk()

    # (c) chains of equal hashes behind the aliases.  Three grams x1 x2 x1: the slot holds x2 when the second x1 is probed --
    # a miss, where a chain resolved to its first lane would hit; then x2 again, a miss on x1.  And x1 x2 x2: a hit, 4 back.
    h, p1, p2 = k.hashes()
    x1, x2 = k.gram(h), k.gram(h)
    k.lead()
    k.chunk(), k.put(p1), k.put(p2), k.put(x1), k.put(x2), k.put(x1), k.put(x2), k.fresh(), k.chunk()
    h, p1, p2 = k.hashes()
    x1, x2 = k.gram(h), k.gram(h)
    k.lead()
    k.chunk(), k.put(p1), k.put(p2), k.put(x1), k.put(x2), k.put(x2), k.fresh(), k.chunk()

    # (d) at the window's ends.  Lane 0 has no earlier lane; lanes 1 and 2 need overlapping grams (overlapping()); lane 8 is
    # the first that planted grams reach; lane 63's gram lies across the window's end.
    for s in (1, 2):
        b = overlapping(k.bits, s, seed + s)
        if b is not None:
            k.lead()
            k.put(b), k.fresh(2 - s), k.chunk()
    h, p1, p2 = k.hashes()
    u = k.gram(h) + k.fresh_bytes(4)
    k.planted(u)
    k.lead()
    k.put(p1), k.put(p2), k.put(u), k.chunk()
    h, p1, p2 = k.hashes()
    u = k.gram(h) + k.fresh_bytes(4)
    k.planted(u)
    k.lead(3)
    for _ in range(6):
        k.chunk()
    k.fresh(), k.put(p1), k.put(p2), k.put(u), k.chunk()

    # (e) aliased and saturated: the planted string matches for 40 and for 80 bytes (one copy element, and two)
    for ln in (40, 80):
        h, p1, p2 = k.hashes()
        s = k.gram(h) + k.fresh_bytes(ln - 4)
        k.planted(s)
        k.lead()
        k.chunk(), k.put(p1), k.put(p2), k.put(s), k.fresh(), k.chunk()

    # (f) below the cursor: a copy of 24 bytes from lane 56 of the window in front covers the aliases and the lane; a later
    # lane with the same gram has its partner below the cursor and hits the planted one
    h, p1, p2 = k.hashes()
    x = k.gram(h)
    t = k.fresh_bytes(8) + p1 + p2 + x + k.fresh_bytes(4)
    k.planted(t)
    k.lead()
    for _ in range(7):
        k.chunk()
    k.put(t), k.fresh(), k.put(x), k.fresh(), k.chunk()

    k.to_lane(0)
    assert len(k.buf) + 256 <= n, (len(k.buf), n)          # every window above is one the stream form takes
    while len(k.buf) + 8 <= n:
        k.chunk()
    k.fresh(n - len(k.buf))
    return bytes(k.buf)


def small_alphabet_text(n=32768, seed=5):
    """words of 2-6 letters over six letters, from a vocabulary of 300: few distinct grams, each very frequent, so that a
    window's lanes share slots -- and hashes -- all the time"""
    r = np.random.default_rng(seed)
    words = [bytes(r.choice(np.frombuffer(b"aeinst", dtype=np.uint8), size=int(r.integers(2, 7)))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += words[int(r.integers(0, 300))] + b" "
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, data, block size)]: the constructed block for each block size and each alias bit, and the text at both"""
    out = []
    for n in BLOCKS:
        for abit in ("top", 8):
            out.append(("built/%d/%s" % (n, abit), _build(n, abit, seed=n + (0 if abit == "top" else 1)), n))
    text = small_alphabet_text()
    out += [("text/%d" % n, text, n) for n in BLOCKS]
    return out
