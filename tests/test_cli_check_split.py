"""dpu_snappy -R -T -S in host mode (no -d): the host codec ignores -S, as it does for decoding, so the run is that of -R -T --
the same Check: line, the same exit status; -S takes no <unit_len> beside -T; without -R it is refused as before."""
import os

from conftest import GOLDEN
import raw_cases as rc
from test_cli import cli, run  # noqa: F401  (the module's fixture and helpers)
from test_cli_check import check_line

RAW = os.path.join(GOLDEN, "raw", "terror2.raw_snappy")


def test_cli_check_split_host_mode_ignores_S(cli, tmp_path):
    r, plain = run(cli, "-R", "-T", "-S", "-i", RAW), run(cli, "-R", "-T", "-i", RAW)
    assert r.returncode == plain.returncode == 0, r.stderr
    assert check_line(r) == check_line(plain) == "Check: OK, 105438 bytes"
    cut = tmp_path / "cut.raw_snappy"
    cut.write_bytes(rc.fixture_stream("terror2")[:40000])
    r, plain = run(cli, "-T", "-S", "-R", "-i", str(cut)), run(cli, "-T", "-R", "-i", str(cut))
    assert r.returncode == plain.returncode == 1 and check_line(r) == check_line(plain) == "Check: INVALID"
    assert sorted(os.listdir(tmp_path)) == ["cut.raw_snappy"]


def test_cli_check_split_refuses_a_unit_length_and_a_framed_file(cli, tmp_path):
    for args in (("-R", "-T", "-S", "1024"), ("-R", "-T", "-S65536"), ("-R", "-S", "512", "-T"), ("-d", "-R", "-T", "-S", "4096")):
        r = run(cli, *args, "-i", RAW)
        assert r.returncode not in (0, 1) and "unit_len" in r.stderr and "Check:" not in r.stdout, (args, r.stderr)
    for args in (("-T", "-S"), ("-c", "-R", "-S", "-T")):
        r = run(cli, *args, "-i", RAW)
        assert r.returncode not in (0, 1) and r.stderr.strip() and "Check:" not in r.stdout, (args, r.stderr)
    assert os.listdir(tmp_path) == []
