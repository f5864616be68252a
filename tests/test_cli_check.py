"""dpu_snappy -T in host mode (no -d): is a compressed file intact?  No output file; one `Check:` line, the usual timing lines,
exit status 0 for OK and 1 for INVALID.  The host's verdict is snappy_host.c's own decoder's, block by block."""
import os
import re

import pytest

import k2_window_cases as kc
import raw_cases as rc
from conftest import GOLDEN, GOLDEN_PAIRS, golden_bytes
from test_cli import LINES, cli, run  # noqa: F401  (the module's fixture and helpers)

TIMING = LINES[4:]


def check_line(r):
    """the one Check: line of a -T run, after the stdout contract: input file, Check, the seven timing lines"""
    lines = [ln for ln in r.stdout.strip().splitlines() if not ln.startswith("GPU ") and ln != "bad offset!"]
    assert re.fullmatch(LINES[0], lines[0]), r.stdout
    assert lines[1].startswith("Check: "), r.stdout
    assert len(lines) == 2 + len(TIMING), r.stdout
    for pat, line in zip(TIMING, lines[2:]):
        assert re.fullmatch(pat, line), (pat, line)
    return lines[1]


def damaged_copy(stream, blocks):
    """the first tag of each of `blocks` turned into a 64-byte copy: nothing to copy from at the start of a block"""
    _, _, offs = kc._offsets(stream)
    b = bytearray(stream)
    for k in blocks:
        b[offs[k] + 4] = 0xFF
    return bytes(b), offs


@pytest.mark.parametrize("name", GOLDEN_PAIRS)
def test_cli_check_goldens_are_ok(cli, tmp_path, name):
    r = run(cli, "-T", "-i", os.path.join(GOLDEN, name + ".snappy"))
    assert r.returncode == 0, r.stderr
    _, _, offs = kc._offsets(golden_bytes(name + ".snappy"))
    assert check_line(r) == "Check: OK, %d blocks" % len(offs)


def test_cli_check_writes_no_file_and_refuses_an_output(cli, tmp_path):
    import subprocess
    src = os.path.join(GOLDEN, "terror2.snappy")
    r = subprocess.run([cli, "-T", "-i", src], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and os.listdir(tmp_path) == []
    for extra in (("-o", str(tmp_path / "o")), ("-c",), ("-r", "0:10"), ("-t", "5")):
        r = run(cli, "-T", *extra, "-i", src)
        assert r.returncode not in (0, 1) and r.stderr.strip() and "Check:" not in r.stdout, extra
    assert os.listdir(tmp_path) == []


def test_cli_check_damaged_copy(cli, tmp_path):
    stream = golden_bytes("terror2.snappy")
    bad, offs = damaged_copy(stream, (1, 3))
    src = tmp_path / "bad.snappy"
    src.write_bytes(bad)
    r = run(cli, "-T", "-i", str(src))
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert check_line(r) == "Check: INVALID, 2 of 4 blocks, first bad block 1 at offset %d" % offs[1]
    # a broken chain: the file cut inside block 2, and two bytes behind the last block
    src.write_bytes(stream[:offs[2] + 100])
    r = run(cli, "-T", "-i", str(src))
    assert r.returncode == 1 and check_line(r) == "Check: INVALID, 1 of 4 blocks, first bad block 2 at offset %d" % offs[2]
    src.write_bytes(stream + b"xx")
    r = run(cli, "-T", "-i", str(src))
    assert r.returncode == 1 and check_line(r) == "Check: INVALID, 1 of 4 blocks, first bad block 3 at offset %d" % offs[3]
    src.write_bytes(b"\xff\xff")
    r = run(cli, "-T", "-i", str(src))
    assert r.returncode == 1 and check_line(r) == "Check: INVALID, 1 of 0 blocks, first bad block 0 at offset 0"
    # an empty container is intact
    src.write_bytes(bytes.fromhex("00808002"))
    r = run(cli, "-T", "-i", str(src))
    assert r.returncode == 0 and check_line(r) == "Check: OK, 0 blocks"


def test_cli_check_raw_fixture_and_its_cut_versions(cli, tmp_path):
    for name in rc.FIXTURES:
        r = run(cli, "-T", "-R", "-i", os.path.join(GOLDEN, "raw", name + ".raw_snappy"))
        assert r.returncode == 0, (name, r.stderr)
        assert check_line(r) == "Check: OK, %d bytes" % len(rc.fixture_plain(name))
    s = rc.fixture_stream("terror2")
    src = tmp_path / "cut.raw_snappy"
    for cut in (len(s) - 1, len(s) // 2, 3, 1, 0):
        src.write_bytes(s[:cut])
        r = run(cli, "-T", "-R", "-i", str(src))
        assert r.returncode == 1 and check_line(r) == "Check: INVALID", cut
    for name, v in rc.damaged_vectors().items():
        src.write_bytes(v)
        r = run(cli, "-T", "-R", "-i", str(src))
        assert r.returncode == 1 and check_line(r) == "Check: INVALID", name
    assert os.listdir(tmp_path) == ["cut.raw_snappy"]
