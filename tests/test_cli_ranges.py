"""dpu_snappy -r OFFSET:LENGTH in host mode (no -d): only the blocks the range touches are decoded, and the output file
holds exactly those bytes; the argument errors end with a message and a non-zero exit."""
import os

import numpy as np
import pytest

import ranges_cases as rc
from conftest import GOLDEN, GOLDEN_PAIRS, golden_bytes
from test_cli import LINES, check_stdout_contract, cli, run  # noqa: F401  (the module's fixture and helpers)

assert len(LINES) == 11


@pytest.mark.parametrize("name", GOLDEN_PAIRS)
def test_cli_range_host_matches_oracle_slices(cli, tmp_path, name):
    plain = golden_bytes(name + ".txt")
    c = rc.Container(plain, golden_bytes(name + ".snappy"))
    ranges = rc.boundary_ranges(c.total, c.block_size, seed=3, random_count=4)
    for k, (off, n) in enumerate(ranges):
        out = tmp_path / f"{name}.{k}"
        r = run(cli, "-r", f"{off}:{n}", "-i", os.path.join(GOLDEN, name + ".snappy"), "-o", str(out))
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == plain[off:off + n], (off, n)
        if n:
            check_stdout_contract(r.stdout)
            assert f"Decompressed {n} bytes to: {out}" in r.stdout


def test_cli_range_xml_stand_in(cli, tmp_path):
    """xml.snappy (5.3 MB, 164 blocks): ranges deep in the chain, against the full host decode."""
    full = tmp_path / "xml.full"
    r = run(cli, "-i", os.path.join(GOLDEN, "xml.snappy"), "-o", str(full))
    assert r.returncode == 0, r.stderr
    plain = full.read_bytes()
    rng = np.random.default_rng(11)
    for k in range(6):
        off = int(rng.integers(0, len(plain) - 1))
        n = int(min(len(plain) - off, rng.integers(1, 200_000)))
        out = tmp_path / f"xml.{k}"
        r = run(cli, "-r", f"{off}:{n}", "-i", os.path.join(GOLDEN, "xml.snappy"), "-o", str(out))
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == plain[off:off + n]


@pytest.mark.parametrize("arg", ["10", "10:", ":10", "a:10", "10:b", "10:5x", "-1:5", "5:-1", ""])
def test_cli_range_malformed_argument(cli, tmp_path, arg):
    r = run(cli, "-r", arg, "-i", os.path.join(GOLDEN, "alice.snappy"), "-o", str(tmp_path / "o"))
    assert r.returncode != 0 and r.stderr.strip()
    assert not (tmp_path / "o").exists()


def test_cli_range_with_compress_and_beyond_the_file(cli, tmp_path):
    r = run(cli, "-c", "-r", "0:10", "-i", os.path.join(GOLDEN, "alice.txt"), "-o", str(tmp_path / "c"))
    assert r.returncode != 0 and "-c" in r.stderr
    assert not (tmp_path / "c").exists()
    total = len(golden_bytes("alice.txt"))
    for arg in (f"{total}:1", f"0:{total + 1}", f"{(1 << 64) - 1}:2"):
        r = run(cli, "-r", arg, "-i", os.path.join(GOLDEN, "alice.snappy"), "-o", str(tmp_path / "b"))
        assert r.returncode != 0 and r.stderr.strip(), arg
        assert not (tmp_path / "b").exists()
