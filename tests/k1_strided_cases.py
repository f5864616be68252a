"""Inputs of the strided-scan tests (tests/test_k1_strided_emulated.py, tests/test_gpu_k1_strided.py): data on which the
reference's skip heuristic (snappy_compress.c:336-348) widens its stride, so that K1's bulk form scans in batches of 64
probes (csrc/snappy_kernels.hpp: strided_scan_batch).  Every input is compared with the oracle byte for byte."""
import functools

import numpy as np

import datagen
from conftest import golden_bytes

PLANTED_BLOCK = 32768
PLANTED_BLOCKS = 64


@functools.lru_cache(maxsize=None)
def planted(blocks=PLANTED_BLOCKS, seed=7):
    """`blocks` blocks of 32 KiB of random bytes, each with six stretches of 40-199 bytes copied from [0, 12000) to
    [14000, end): the scan runs at a wide stride through noise and meets a match there -- a batch that ends on a hit, from
    which the match is taken and the scan starts again at stride 1."""
    r = np.random.default_rng(seed)
    out = []
    for _ in range(blocks):
        blk = r.integers(0, 256, size=PLANTED_BLOCK, dtype=np.uint8)
        for _ in range(6):
            ln = int(r.integers(40, 200))
            src = int(r.integers(0, 12000 - ln))
            dst = int(r.integers(14000, PLANTED_BLOCK - ln))
            blk[dst:dst + ln] = blk[src:src + ln]
        out.append(blk)
    return np.concatenate(out).tobytes()


@functools.lru_cache(maxsize=None)
def cases(planted_blocks=8):
    """[(name, data, block size)]: (a) one block of noise at 32768 and at 65535 (positions above 32767 in u16 slots); (b) noise
    of every length 600..663 as one block (1,024 table entries: shared slots within a batch are common, and 64 consecutive
    lengths walk the limit test across the lanes); (c) the planted construction; (d) text and noise interleaved (the stride
    ramps up and back to 1, with hand-over to and from the stream form); (e) noise followed by text and the reverse."""
    text = golden_bytes("plrabn12.txt")
    out = [("noise/32768", datagen.random_bytes(32768, seed=11), 32768),
           ("noise/65535", datagen.random_bytes(65535, seed=12), 65535)]
    out += [("noise/%d" % n, datagen.random_bytes(n, seed=1000 + n), n) for n in range(600, 664)]
    out.append(("planted", planted()[:planted_blocks * PLANTED_BLOCK], PLANTED_BLOCK))
    mixed = datagen.text_random_interleave(text, 150_000)
    out += [("interleave/32768", mixed, 32768), ("interleave/4097", mixed, 4097)]
    noise, prose = datagen.random_bytes(20_000, seed=13), golden_bytes("alice.txt")[:12_768]
    out += [("noise+text", noise + prose, 32768), ("text+noise", prose + noise, 32768)]
    return out
