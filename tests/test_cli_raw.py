"""dpu_snappy -R in host mode (no -d): the original ("raw") Snappy format.  -c -R writes exactly tools/to_raw_snappy.convert
of what -c writes for the same file; -R decodes third-party streams (literals above 64 KiB, references across any boundary)
and refuses damaged ones; -R with -r or -w is a usage error."""
import os

import pytest

import raw_cases as rc
from conftest import GOLDEN, GOLDEN_PAIRS, golden_bytes
from test_cli import LINES, check_stdout_contract, cli, run  # noqa: F401  (the module's fixture and helpers)

assert len(LINES) == 11


@pytest.mark.parametrize("bs", [64, 1000, 32768, 65535])
@pytest.mark.parametrize("name", GOLDEN_PAIRS)
def test_cli_raw_compress_is_the_converted_framed_stream(cli, tmp_path, name, bs):
    src = os.path.join(GOLDEN, name + ".txt")
    raw, framed, back = tmp_path / "raw", tmp_path / "framed", tmp_path / "back"
    r = run(cli, "-c", "-R", "-b", str(bs), "-i", src, "-o", str(raw))
    assert r.returncode == 0, r.stderr
    check_stdout_contract(r.stdout)
    assert run(cli, "-c", "-b", str(bs), "-i", src, "-o", str(framed)).returncode == 0
    got = raw.read_bytes()
    assert got == rc.trs.convert(framed.read_bytes())
    if bs == 32768:
        assert got == rc.trs.convert(golden_bytes(name + ".snappy"))
    assert rc.trs.decode_raw(got) == golden_bytes(name + ".txt")
    r = run(cli, "-R", "-i", str(raw), "-o", str(back))
    assert r.returncode == 0, r.stderr
    check_stdout_contract(r.stdout)
    assert back.read_bytes() == golden_bytes(name + ".txt")


def test_cli_raw_decodes_fixtures_and_vectors(cli, tmp_path):
    streams = {n: rc.fixture_stream(n) for n in rc.FIXTURES}
    streams.update(rc.intact_vectors())
    for name, s in streams.items():
        src, out = tmp_path / (name + ".raw_snappy"), tmp_path / (name + ".out")
        src.write_bytes(s)
        r = run(cli, "-R", "-i", str(src), "-o", str(out))
        assert r.returncode == 0, (name, r.stderr)
        assert out.read_bytes() == rc.trs.decode_raw(s), name
    for name in rc.FIXTURES:
        assert (tmp_path / (name + ".out")).read_bytes() == rc.fixture_plain(name)


def test_cli_raw_refuses_damaged_streams(cli, tmp_path):
    for name, s in rc.damaged_vectors().items():
        src, out = tmp_path / (name + ".raw_snappy"), tmp_path / (name + ".out")
        src.write_bytes(s)
        r = run(cli, "-R", "-i", str(src), "-o", str(out))
        assert r.returncode != 0 and not out.exists(), name


def test_cli_raw_empty_file(cli, tmp_path):
    src, raw, back = tmp_path / "empty", tmp_path / "raw", tmp_path / "back"
    src.write_bytes(b"")
    assert run(cli, "-c", "-R", "-i", str(src), "-o", str(raw)).returncode == 0
    assert raw.read_bytes() == b"\x00"
    assert run(cli, "-R", "-i", str(raw), "-o", str(back)).returncode == 0
    assert back.read_bytes() == b""


@pytest.mark.parametrize("extra", [("-r", "0:10"), ("-w", "0:PATCH"), ("-c", "-r", "0:10")])
def test_cli_raw_with_range_or_write_is_a_usage_error(cli, tmp_path, extra):
    patch = tmp_path / "patch"
    patch.write_bytes(b"x")
    args = [str(patch).join(a.split("PATCH")) if "PATCH" in a else a for a in extra]
    r = run(cli, "-R", *args, "-i", os.path.join(GOLDEN, "raw", "alice.raw_snappy"), "-o", str(tmp_path / "o"))
    assert r.returncode != 0 and r.stderr.strip()
    assert not (tmp_path / "o").exists()
