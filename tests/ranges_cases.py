"""Range requests and their expected bytes for the range decoder tests (tests/test_ranges_emulated.py on the CPU wave
emulator, tests/test_gpu_ranges.py through the C ABI).  Test infrastructure only: plain Python + the oracle."""
import numpy as np

import oracle_lib as oracle

GUARD = 0xA5          # every byte of a destination buffer outside the ranges' bytes
GAP = 37              # guard bytes in front of every destination (odd: destinations land on every alignment)
OUT_OF_BOUNDS = 2     # SNAPPY_HIP_RANGE_OUT_OF_BOUNDS


class Container:
    """A framed stream with its plaintext and its block offsets (as snappy_hip_index_streams leaves them)."""

    def __init__(self, plain, stream=None, block_size=32768):
        self.plain = plain
        self.stream = stream if stream is not None else oracle.compress(plain, block_size)
        self.total, self.block_size, self.header_len = oracle.read_header(self.stream)
        self.num_blocks = (self.total + self.block_size - 1) // self.block_size if self.total else 0
        self.offsets = oracle.index_blocks(self.stream) if self.num_blocks else np.zeros(0, dtype=np.uint64)
        assert self.total == len(plain)


def boundary_ranges(total, bs, seed, random_count=12):
    """(offset, length) pairs: single bytes on both sides of block boundaries, ranges of 1, 2 and many blocks, the last
    (partial) block, the whole container, length 0 (also at the very end), and seeded random ones."""
    rs = []
    nb = (total + bs - 1) // bs
    for b in sorted({1, 2, nb // 2, nb - 1}):
        if 0 < b < nb:
            rs += [(b * bs - 1, 1), (b * bs, 1), (b * bs - 1, 2)]
    rs += [(0, min(total, bs)), (0, 1), (total - 1, 1)]                       # first block whole, first and last byte
    if nb >= 2:
        rs += [(bs // 2, bs), (bs, min(bs, total - bs))]                       # two blocks partially; the second whole
    if nb >= 3:
        rs += [(bs // 3, total - bs // 3 - 1), (bs, total - bs)]               # many blocks, from a block start to the end
    rs += [((nb - 1) * bs, total - (nb - 1) * bs), (0, total), (5 % total, 0), (total, 0)]   # last block, all, empty ones
    rng = np.random.default_rng(seed)
    for _ in range(random_count):
        off = int(rng.integers(0, total))
        length = int(min(total - off, rng.integers(0, 3 * bs + 2)))
        rs.append((off, length))
    return [(o, n) for o, n in rs if 0 <= o and o + n <= total]


def layout(lengths, gap=GAP):
    """Destination offsets in one buffer: every range behind `gap` guard bytes; returns (offsets, buffer length)."""
    offs, at = [], 0
    for n in lengths:
        at += gap
        offs.append(at)
        at += n
    return offs, at + gap


def check_buffer(buf, expected):
    """buf: the destination buffer; expected: list of (dst offset, length, want) with want = the bytes the range must hold,
    None (the range must not have been written) or "any" (an INVALID range: contents unspecified).  Every byte that no
    range owns must still be GUARD.  Returns a list of problems (empty = all good)."""
    buf = np.asarray(buf, dtype=np.uint8)
    owned = np.zeros(buf.size, dtype=bool)
    problems = []
    for i, (o, n, want) in enumerate(expected):
        if want is None:
            continue
        owned[o:o + n] = True
        if want == "any":
            continue
        got = buf[o:o + n].tobytes()
        if got != want:
            bad = next(k for k in range(n) if got[k] != want[k])
            problems.append(f"range {i}: first wrong byte at {bad} of {n}")
    stray = np.flatnonzero(~owned & (buf != GUARD))
    if stray.size:
        problems.append(f"{stray.size} guard bytes overwritten, first at {int(stray[0])}")
    return problems
