"""Write sets and their expected streams for the container update tests (tests/test_update_emulated.py on the CPU wave
emulator, tests/test_gpu_update.py through the C ABI, tests/test_cli_update.py through the CLI).  Test infrastructure only:
plain Python + the oracle."""
import numpy as np

import oracle_lib as oracle
import ranges_cases as rc

GUARD = 0x5A              # every byte of an output buffer the call must not write
OK, INVALID, OUT_OF_BOUNDS, UNORDERED, REJECTED = 0, 1, 2, 3, 4
KINDS = ("same", "zeros", "random")


def patched(plain, writes):
    """plain with every (offset, data) laid over it."""
    out = bytearray(plain)
    for off, data in writes:
        out[off:off + len(data)] = data
    return bytes(out)


def new_bytes(plain, off, n, kind, seed=0):
    """The three kinds of new bytes: the ones already there (the stream must not change), zeros (blocks shrink to a few
    bytes), seeded random bytes (blocks grow to the slot's worst case)."""
    if kind == "same":
        return plain[off:off + n]
    if kind == "zeros":
        return bytes(n)
    return np.random.default_rng(seed * 1000003 + off).integers(0, 256, n, dtype=np.uint8).tobytes()


def disjoint(ranges):
    """(offset, length) pairs made sorted and disjoint: sorted by offset, a range that starts inside its predecessor is
    cut to start at the predecessor's end (possibly down to length 0)."""
    out, end = [], 0
    for o, n in sorted(ranges):
        e = o + n
        o = max(o, end)
        out.append((o, max(e, o) - o))
        end = max(end, e)
    return out


def write_sets(total, bs, seed, random_count=8):
    """Lists of (offset, length): every boundary range of ranges_cases alone, then sets of them made sorted and disjoint."""
    singles = rc.boundary_ranges(total, bs, seed=seed, random_count=random_count)
    sets = [[r] for r in singles]
    sets.append(disjoint(singles))
    sets.append(disjoint([r for r in singles if r[1] <= 2]))                 # single bytes around the block boundaries only
    sets.append(disjoint(singles[::2]))
    return sets


def dirty_blocks(writes, bs):
    """Indices of the blocks that (offset, length) pairs touch."""
    d = set()
    for o, n in writes:
        if n:
            d.update(range(o // bs, (o + n - 1) // bs + 1))
    return sorted(d)


def expected(container, writes_with_data):
    """(stream, offsets + [len], dirty count) an update must produce."""
    new_plain = patched(container.plain, writes_with_data)
    stream = oracle.compress(new_plain, container.block_size)
    offs = [int(x) for x in oracle.index_blocks(stream)] if container.num_blocks else []
    return stream, offs + [len(stream)], len(dirty_blocks([(o, len(d)) for o, d in writes_with_data], container.block_size))
