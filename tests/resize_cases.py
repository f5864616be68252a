"""Cuts, tails and their expected streams for the container resize tests (tests/test_resize_emulated.py on the CPU wave
emulator, tests/test_gpu_resize.py through the C ABI, tests/test_cli_resize.py through the CLI).  Test infrastructure only:
plain Python + the oracle."""
import numpy as np

import oracle_lib as oracle
import update_cases as uc

GUARD = uc.GUARD
OK, INVALID, OUT_OF_BOUNDS, REJECTED = uc.OK, uc.INVALID, uc.OUT_OF_BOUNDS, uc.REJECTED
KINDS = uc.KINDS


def new_plain(plain, keep_len, segments):
    """The first keep_len bytes of plain followed by the segments' bytes in order."""
    return plain[:keep_len] + b"".join(segments)


def expected(container, keep_len, segments):
    """(stream, offsets + [len], compressed-block count) a resize must produce.  segments: list of bytes."""
    bs = container.block_size
    plain = new_plain(container.plain, keep_len, segments)
    stream = oracle.compress(plain, bs)
    nb = (len(plain) + bs - 1) // bs
    offs = [int(x) for x in oracle.index_blocks(stream)] if nb else []
    return stream, offs + [len(stream)], nb - keep_len // bs


def boundary(total, bs, last=True):
    """A block boundary inside the container (0 < boundary < total) if it has one: the last one, or the middle one."""
    nb = (total + bs - 1) // bs
    if nb < 2:
        return None
    return ((nb - 1) if last else max(1, nb // 2)) * bs


def keep_lens(total, bs, last=True):
    """0, 1, a boundary - 1, the boundary, the boundary + 1, total - 1, total -- those that lie in [0, total], each once."""
    b = boundary(total, bs, last)
    ks = [0, 1] + ([b - 1, b, b + 1] if b is not None else []) + [total - 1, total]
    return sorted({k for k in ks if 0 <= k <= total})


def tail_lens(keep_len, bs):
    """0 bytes, 1 byte, exactly the bytes that fill the block keep_len cuts (a whole block when it cuts none), one more than
    that, and 2.5 blocks (at least 3 bytes), each once."""
    fill = bs - keep_len % bs
    return sorted({0, 1, fill, fill + 1, max(3, bs * 5 // 2)})


def tail_bytes(plain, keep_len, n, kind, seed=0):
    """The three kinds of new bytes of update_cases.new_bytes; "same" = the plaintext behind keep_len going on (around its
    end), so that a tail of total - keep_len bytes gives the old stream again."""
    if kind == "same":
        src = plain[keep_len:] + plain if plain else bytes(1)
        return (src * (n // len(src) + 1))[:n]
    return uc.new_bytes(plain, keep_len, n, kind, seed)


def split(data, lengths):
    """data cut into pieces of the given lengths in turn (cyclically; a length of 0 gives an empty piece) until it is used up."""
    out, at, i = [], 0, 0
    while at < len(data):
        n = lengths[i % len(lengths)]
        out.append(data[at:at + n])
        at += n
        i += 1
        assert i < 10 * len(data) + 10 * len(lengths), "lengths of 0 only"
    return out


def mixed_lengths(count, seed, most=40):
    """`count` seeded segment lengths of 0 .. most bytes, every fifth one 0."""
    ls = np.random.default_rng(seed).integers(1, most + 1, count)
    ls[::5] = 0
    return [int(x) for x in ls]


def rejected_cases(c):
    """(keep_len, segments, new_total_len or None for keep_len + the lengths, statuses, capacity or None): each cause alone --
    whatever else the call says is right -- then two mixed."""
    big = (1 << 64) - 1
    keep = 10000
    good = [b"abc", b"defgh"]
    null = (b"", 3, True)
    return [
        (c.total + 1, good, None, [0, 0], None),                                       # keep_len beyond the container, the sum right
        (c.total + 1, [], None, [], None),                                             # ... and with no segment at all
        (keep, good, keep + 9, [0, 0], None),                                          # new_total_len one more than the sum
        (keep, good, keep + 7, [0, 0], None),                                          # ... and one less
        (keep, [good[0], null, good[1]], None, [0, OUT_OF_BOUNDS, 0], None),        # a null src with length > 0, the sum right
        (keep, [good[0], (b"", big, False), (b"", 12, False)], keep + 3 + 11, [0, 0, 0], None),   # the 64-bit sum overflows to keep + 14
        (keep, [(b"", 1 << 32, False)], keep, [0], None),                              # a plain mismatch: the sum is compared in 64 bits
        # a length of 2^32 is counted as 2^32 - 1, which IS new_total_len here: only the length's own check rejects it
        (0, [b"", (b"", 1 << 32, False), b""], 0xffffffff, [0, 0, 0], 1000),
        (c.total + 1, [good[0], null], keep, [0, OUT_OF_BOUNDS], None),             # two mixed
        (keep, [null, good[0]], keep + 100, [OUT_OF_BOUNDS, 0], None),
    ]
