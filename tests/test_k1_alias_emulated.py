"""CPU tests of the aliases of the stream form's duplicate analysis (csrc/snappy_k1_stream.hpp: stream_analyse resolves a
lane that has an alias in front of it in both tables -- clears it where no earlier lane has its hash, keeps it for the walk
where one has): the unmodified kernel source under the wave emulator against the oracle, byte for byte, on windows built to
alias (tests/k1_alias_cases.py), for every K1 kernel that carries the stream form, with LDS executing in lane order and, with
EMU_LDS_UNORDERED=1, in no order (the analysis then falls back and keeps every sharer)."""
import functools
import os
import subprocess
import sys

import pytest

import k1_alias_cases as cases
import oracle_lib as oracle

# stream-form compress variants (tests/test_emulated_kernels.py): the LDS-table kernel (512-slot analysis), the global-table
# kernel behind the slot filter, behind the slot cache of 512 slots (the product's) and of 256 (256-slot analysis all three)
VARIANTS = (3501, 13503, 43503, 53503)
BY_NAME = {name: (data, bs) for name, data, bs in cases.cases()}
HERE = os.path.dirname(os.path.abspath(__file__))

# what the child prints per (variant, input): same as the oracle?, then stream and alias statistics
_CHILD = """
import sys
sys.path.insert(0, %r)
import emu_k1_alias_lib as emu, k1_alias_cases as cases, oracle_lib as oracle
for name, data, bs in cases.cases():
    ref = oracle.compress(data, bs)
    for cv in %r:
        emu.stream_stats(), emu.alias_stats()
        got = emu.compress(data, bs, cv)
        print(name, cv, int(got == ref), *emu.stream_stats(), *emu.alias_stats())
"""


@functools.lru_cache(maxsize=None)
def _run(unordered):
    """{(input, variant): (same as the oracle's, stream statistics, alias statistics)} of one emulator process: the order in
    which LDS executes is read from the environment once per process"""
    env = dict(os.environ)
    env.pop("EMU_LDS_UNORDERED", None)
    if unordered:
        env["EMU_LDS_UNORDERED"] = "1"
    out = subprocess.run([sys.executable, "-c", _CHILD % (HERE, VARIANTS)], env=env, check=True, capture_output=True, text=True).stdout
    res = {}
    for line in out.splitlines():
        f = line.split()
        v = [int(x) for x in f[2:]]
        res[(f[0], int(f[1]))] = (bool(v[0]), tuple(v[1:17]), tuple(v[17:33]))
    assert len(res) == len(BY_NAME) * len(VARIANTS)
    return res


@pytest.mark.parametrize("unordered", (False, True), ids=("in_order", "unordered"))
@pytest.mark.parametrize("cv", VARIANTS)
def test_aliased_windows_are_the_oracles(cv, unordered):
    res = _run(unordered)
    for name in BY_NAME:
        assert res[(name, cv)][0], (cv, name, unordered)


def test_oracle_streams_of_the_cases_decode():
    import emu_k1_alias_lib as emu
    for name, (data, bs) in BY_NAME.items():
        ref = oracle.compress(data, bs)
        total, got_bs, hdr = oracle.read_header(ref)
        st, out = emu.decompress(ref, total, got_bs, hdr)
        assert st == 0 and out == data, name


def test_the_analysis_loop_ended_in_every_way():
    """The condition under which the byte comparisons above mean something: aliased lanes were found, and the loop over them
    ended in each of its ways -- cleared (no earlier lane with the hash), kept (there is one), and not run at all because
    the window fell back -- at least 5 times each; the windows of the constructed blocks were taken by the stream form; a
    lane that was cleared causes no settle, so in order no long-way settle of an aliased lane finds nothing."""
    ordered, unordered = _run(False), _run(True)
    for cv in VARIANTS:
        tot = [0] * 16
        for name in BY_NAME:
            same, stream, alias = ordered[(name, cv)]
            assert same, (cv, name)
            tot = [a + b for a, b in zip(tot, alias)]
            if name.startswith("built/"):
                assert stream[0] >= 20, (cv, name, stream)          # windows taken by the stream form
        entered, cleared, kept, fallback, by_cx = tot[:5]
        print("variant %d in order: entered %d, cleared %d, kept %d, fallback windows %d, settles of kept lanes %d, long-way settles that found nothing %d"
              % (cv, entered, cleared, kept, fallback, by_cx, tot[9]))
        assert entered == cleared + kept
        assert cleared >= 5 and kept >= 5, (cv, tot)
        assert fallback == 0, (cv, tot)
        assert by_cx <= kept, (cv, tot)
        fb = sum(unordered[(name, cv)][2][3] for name in BY_NAME)
        print("variant %d unordered: fallback windows %d" % (cv, fb))
        assert fb >= 5, (cv, fb)
