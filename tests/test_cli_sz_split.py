"""dpu_snappy -z -S: the .sz reader with the chunk chain of a large file walked by many wavefronts.  On the CPU: the refusals
(-S takes no value beside -z, and does not go with -c) and host mode, which ignores -S as it does beside -R.  The -d cases
(marked gpu) hold -d -z -S and -d -z -T -S to -d -z and -d -z -T on intact and damaged files, small and of several segments."""
import re

import pytest

import sz_cases as sz
from test_cli import cli, run  # noqa: F401  (the module's fixture and helpers)


def check_line(r):
    m = re.search(r"^Check: .*$", r.stdout, re.M)
    return m.group(0) if m else None


@pytest.mark.parametrize("extra", [("-S", "4096"), ("-S4096",), ("-S", "-c"), ("-c", "-S"), ("-T", "-S", "256"), ("-S", "-R"), ("-S", "-W")])
def test_cli_sz_split_usage_errors(cli, tmp_path, extra):
    src = tmp_path / "in.sz"
    src.write_bytes(sz.IDENTIFIER)
    for mode in ((), ("-d",)):
        r = run(cli, *mode, "-z", *extra, "-i", str(src)) if "-T" in extra else run(cli, *mode, "-z", *extra, "-i", str(src), "-o", str(tmp_path / "o"))
        assert r.returncode not in (0, 1) and r.stderr.strip() and "Check:" not in r.stdout, (mode, extra, r.stderr)
        if extra[0].startswith("-S4") or extra[-1].isdigit():
            assert "takes no" in r.stderr, r.stderr
    assert not (tmp_path / "o").exists()


def test_cli_sz_split_host_mode_ignores_S(cli, tmp_path):
    s, plain = sz.intact_streams()["pyarrow_65536"]
    src, out = tmp_path / "p.sz", tmp_path / "p.out"
    src.write_bytes(s)
    r = run(cli, "-z", "-S", "-i", str(src), "-o", str(out))
    assert r.returncode == 0 and out.read_bytes() == plain, r.stderr
    r, same = run(cli, "-z", "-T", "-S", "-i", str(src)), run(cli, "-z", "-T", "-i", str(src))
    assert r.returncode == same.returncode == 0 and check_line(r) == check_line(same) == "Check: OK, %d bytes" % len(plain)
    bad = tmp_path / "bad.sz"
    bad.write_bytes(sz.damaged_streams()["truncated_by_1"])
    r = run(cli, "-z", "-S", "-T", "-i", str(bad))
    assert r.returncode == 1 and check_line(r) == "Check: INVALID"


@pytest.fixture(scope="module")
def big():
    plain = sz.text_random_mix(3 * 512 * 1024, 78)            # three segments at the default
    return sz.write_sz_pyarrow(plain, 65536), plain


@pytest.mark.gpu
def test_cli_sz_split_gpu_reads_what_the_base_mode_reads(cli, tmp_path, big):
    s, plain = big
    assert len(s) > 1 << 20
    small, small_plain = sz.intact_streams()["padding_and_skippable"]
    for k, (stream, want) in enumerate(((s, plain), (small, small_plain))):
        src, a, b = tmp_path / ("in%d.sz" % k), tmp_path / ("a%d" % k), tmp_path / ("b%d" % k)
        src.write_bytes(stream)
        r = run(cli, "-d", "-z", "-S", "-i", str(src), "-o", str(a))
        assert r.returncode == 0, r.stderr
        assert run(cli, "-d", "-z", "-i", str(src), "-o", str(b)).returncode == 0
        assert a.read_bytes() == b.read_bytes() == want
        r, same = run(cli, "-d", "-z", "-T", "-S", "-i", str(src)), run(cli, "-d", "-z", "-T", "-i", str(src))
        assert r.returncode == same.returncode == 0 and check_line(r) == check_line(same) == "Check: OK, %d bytes" % len(want)


@pytest.mark.gpu
def test_cli_sz_split_gpu_refuses_what_the_base_mode_refuses(cli, tmp_path, big):
    s, _ = big
    damaged = sz.damaged_streams()
    files = {name: damaged[name] for name in ("crc_word_bit_chunk2", "reserved_unskippable_02")}
    files["large_payload_bit_in_the_last_segment"] = s[:-30000] + bytes([s[-30000] ^ 4]) + s[-29999:]
    files["large_truncated"] = s[:-1]
    for name, stream in files.items():
        src, out = tmp_path / (name + ".sz"), tmp_path / (name + ".out")
        src.write_bytes(stream)
        r, same = run(cli, "-d", "-z", "-S", "-i", str(src), "-o", str(out)), run(cli, "-d", "-z", "-i", str(src), "-o", str(out))
        assert r.returncode == same.returncode != 0 and not out.exists(), name
        r, same = run(cli, "-d", "-z", "-T", "-S", "-i", str(src)), run(cli, "-d", "-z", "-T", "-i", str(src))
        assert r.returncode == same.returncode == 1 and check_line(r) == check_line(same) == "Check: INVALID", name
