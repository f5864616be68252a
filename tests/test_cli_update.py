"""dpu_snappy -w OFFSET:PATCHFILE in host mode (no -d): only the blocks the patch touches are decoded and compressed again,
and the output file is byte for byte the oracle's stream for the patched plaintext; the argument errors end with a message,
a non-zero exit and no output file."""
import os

import pytest

import oracle_lib as oracle
import ranges_cases as rc
import update_cases as uc
from conftest import GOLDEN, GOLDEN_PAIRS, golden_bytes
from test_cli import LINES, check_stdout_contract, cli, run  # noqa: F401  (the module's fixture and helpers)

assert len(LINES) == 11


@pytest.mark.parametrize("name", GOLDEN_PAIRS)
def test_cli_update_host_matches_oracle(cli, tmp_path, name):
    plain = golden_bytes(name + ".txt")
    c = rc.Container(plain, golden_bytes(name + ".snappy"))
    ranges = rc.boundary_ranges(c.total, c.block_size, seed=4, random_count=4)
    for k, (off, n) in enumerate(ranges):
        kind = uc.KINDS[k % 3]
        patch = uc.new_bytes(plain, off, n, kind, seed=k)
        pf = tmp_path / f"{name}.{k}.patch"
        pf.write_bytes(patch)
        out = tmp_path / f"{name}.{k}"
        r = run(cli, "-w", f"{off}:{pf}", "-i", os.path.join(GOLDEN, name + ".snappy"), "-o", str(out))
        assert r.returncode == 0, r.stderr
        got = out.read_bytes()
        assert got == oracle.compress(uc.patched(plain, [(off, patch)]), c.block_size), (off, n, kind)
        if kind == "same":
            assert got == c.stream
        check_stdout_contract(r.stdout)
        assert f"Compressed {len(got)} bytes to: {out}" in r.stdout


@pytest.mark.parametrize("arg", ["10", "10:", ":patch", "a:patch", "-1:patch", ""])
def test_cli_update_malformed_argument(cli, tmp_path, arg):
    (tmp_path / "patch").write_bytes(b"xyz")
    r = run(cli, "-w", arg.replace("patch", str(tmp_path / "patch")), "-i", os.path.join(GOLDEN, "alice.snappy"), "-o", str(tmp_path / "o"))
    assert r.returncode != 0 and r.stderr.strip()
    assert not (tmp_path / "o").exists()


def test_cli_update_with_compress_or_range_missing_patch_and_beyond_the_file(cli, tmp_path):
    pf = tmp_path / "patch"
    pf.write_bytes(b"0123456789")
    r = run(cli, "-c", "-w", f"0:{pf}", "-i", os.path.join(GOLDEN, "alice.txt"), "-o", str(tmp_path / "c"))
    assert r.returncode != 0 and "-c" in r.stderr
    r = run(cli, "-r", "0:10", "-w", f"0:{pf}", "-i", os.path.join(GOLDEN, "alice.snappy"), "-o", str(tmp_path / "c"))
    assert r.returncode != 0 and "-r" in r.stderr
    assert not (tmp_path / "c").exists()
    r = run(cli, "-w", f"0:{tmp_path / 'missing'}", "-i", os.path.join(GOLDEN, "alice.snappy"), "-o", str(tmp_path / "m"))
    assert r.returncode != 0 and r.stderr.strip()
    assert not (tmp_path / "m").exists()
    total = len(golden_bytes("alice.txt"))
    for off in (total - 9, total, (1 << 64) - 1):
        r = run(cli, "-w", f"{off}:{pf}", "-i", os.path.join(GOLDEN, "alice.snappy"), "-o", str(tmp_path / "b"))
        assert r.returncode != 0 and r.stderr.strip(), off
        assert not (tmp_path / "b").exists()
    # a damaged container: the chain does not end at the file's end
    bad = tmp_path / "bad.snappy"
    bad.write_bytes(golden_bytes("terror2.snappy")[:-5])
    r = run(cli, "-w", f"0:{pf}", "-i", str(bad), "-o", str(tmp_path / "d"))
    assert r.returncode != 0 and "Encountered Snappy error" in r.stderr
    assert not (tmp_path / "d").exists()
    assert "-w" in run(cli).stderr                               # the usage line names it
