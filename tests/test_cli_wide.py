"""dpu_snappy -W in host mode (no -d): the host codec ignores -W, as it ignores -S; a <waves> outside 2, 4, 8, 16 is a usage
error that names -W; and include/snappy_hip.h declares the wide calls (tests/test_abi_symbols.py then holds their export)."""
import os
import re

import pytest

from conftest import GOLDEN, ROOT, golden_bytes
from test_cli import check_stdout_contract, cli, run  # noqa: F401  (the module's fixture and helpers)


@pytest.mark.parametrize("flag", [("-W",), ("-W4",), ("-W", "16"), ("-W2",)])
def test_host_mode_accepts_and_ignores_wide(cli, tmp_path, flag):
    out = tmp_path / "o.txt"
    r = run(cli, *flag, "-i", os.path.join(GOLDEN, "terror2.snappy"), "-o", str(out))
    assert r.returncode == 0, r.stderr
    check_stdout_contract(r.stdout)                          # the reference's output lines, unchanged
    assert out.read_bytes() == golden_bytes("terror2.txt")


@pytest.mark.parametrize("flag", [("-W", "3"), ("-W3",), ("-W0",), ("-W", "32"), ("-W4x",)])
def test_a_bad_waves_value_is_a_usage_error_that_names_the_flag(cli, tmp_path, flag):
    out = tmp_path / "o.txt"
    r = run(cli, *flag, "-i", os.path.join(GOLDEN, "terror2.snappy"), "-o", str(out))
    assert r.returncode not in (0, 1) and "-W" in r.stderr, (r.returncode, r.stderr)
    assert not out.exists()


@pytest.mark.parametrize("extra", [("-c",), ("-R",), ("-r", "0:10"), ("-t", "5"), ("-T",)])
def test_wide_goes_with_whole_file_decompression_only(cli, tmp_path, extra):
    r = run(cli, "-W", *extra, "-i", os.path.join(GOLDEN, "terror2.snappy"), "-o", str(tmp_path / "o"))
    assert r.returncode not in (0, 1) and "-W" in r.stderr, (extra, r.stderr)


def test_header_declares_the_wide_calls_and_their_limits():
    with open(os.path.join(ROOT, "include", "snappy_hip.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+snappy_hip_decompress_blocks_wide\s*\(", code)
    assert re.search(r"\bsnappy_status\s+snappy_decompress_wide_gpu\s*\(", code)
    assert int(re.search(r"#define\s+SNAPPY_HIP_WIDE_MAX_BLOCK\s+(\d+)u", code).group(1)) == 32768
    assert int(re.search(r"#define\s+SNAPPY_HIP_WIDE_MAX_CSZ\s+(\d+)u", code).group(1)) >= 32 + 32768 + 32768 // 6
    import snappy_hip_binding as shb
    assert (shb.WIDE_MAX_BLOCK, shb.WIDE_MAX_CSZ) == tuple(int(re.search(r"#define\s+SNAPPY_HIP_WIDE_MAX_%s\s+(\d+)u" % n, code).group(1))
                                                          for n in ("BLOCK", "CSZ"))
