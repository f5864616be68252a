"""CPU tests of K1's strided scan batch (csrc/snappy_kernels.hpp: strided_scan_batch, taken by bulk_run where the reference's
skip heuristic, snappy_compress.c:336-348, has widened the stride) and of the long literals it leaves behind (emit_literal):
the unmodified kernel source under the wave emulator against the oracle, byte for byte, on incompressible data and on data
that moves into and out of it, for every shipped K1 form."""
import ctypes
import functools

import pytest

import emu_lib as emu
import k1_strided_cases as cases
import oracle_lib as oracle

# compress variants (tests/test_emulated_kernels.py): LDS table bulk / stream, global table behind the slot filter bulk /
# stream, behind the slot cache of 512 slots bulk / stream, of 256 slots stream
VARIANTS = (2501, 3501, 12503, 13503, 42503, 43503, 53503)
BY_NAME = {name: (data, bs) for name, data, bs in cases.cases()}
GROUPS = {"noise_blocks": ["noise/32768", "noise/65535"], "noise_lengths": ["noise/%d" % n for n in range(600, 664)],
          "planted": ["planted"], "interleave": ["interleave/32768", "interleave/4097"], "edges": ["noise+text", "text+noise"]}


def _stats():
    out = (ctypes.c_ulonglong * 16)()
    emu.lib().emu_stream_stats(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle's stream of one input, computed once, and its round trip through K2 under the emulator."""
    data, bs = BY_NAME[name]
    ref = oracle.compress(data, bs)
    total, got_bs, hdr = oracle.read_header(ref)
    st, out = emu.decompress(ref, total, got_bs, hdr)
    assert st == 0 and out == data, name
    return ref


@functools.lru_cache(maxsize=None)
def _run(cv, name):
    """(K1's stream == the oracle's, statistics of the run)"""
    data, bs = BY_NAME[name]
    _stats()
    got = emu.compress(data, bs, cv)
    return got == _reference(name), _stats()


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("cv", VARIANTS)
def test_strided_scan_is_the_oracles(cv, group):
    for name in GROUPS[group]:
        same, _ = _run(cv, name)
        assert same, (cv, name)


def test_strided_scan_batches_were_taken_and_closed_in_every_way():
    """The condition under which the byte comparisons above mean something: the batch ran, got long, and ended in each of its
    ways.  Statistics 11-15 of the emulator (snappy_kernels.hpp): batches evaluated; closed by a hit, by a shared slot, by the
    limit; full batches of 64 misses."""
    total = [0] * 16
    for cv in VARIANTS:
        for name in BY_NAME:
            same, stats = _run(cv, name)
            assert same, (cv, name)
            total = [a + b for a, b in zip(total, stats)]
    taken, by_hit, by_shared, by_limit, full = total[11:16]
    print("batches %d: hit %d, shared slot %d, limit %d, full %d" % (taken, by_hit, by_shared, by_limit, full))
    assert taken == by_hit + by_shared + by_limit + full
    assert taken >= 200
    assert min(by_hit, by_shared, by_limit, full) >= 5
    # one block of noise: the C model of the reference's scan gives 23.3 batches of up to 64 probes per 32 KiB block; the
    # bound only catches a batch that never gets long
    for cv in VARIANTS:
        _, stats = _run(cv, "noise/32768")
        print("variant %d, 32 KiB of noise: %d batches" % (cv, stats[11]))
        assert 1 <= stats[11] <= 40, (cv, stats[11])
