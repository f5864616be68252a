"""dpu_snappy -z -x <offset>:<length>: a byte range of a .sz stream's plaintext.  Host mode (no -d): the extracted bytes are what
slicing the plaintext gives, for ranges at both ends, across chunk types and over the edge cases of tests/sz_ranges_cases.py; a
range beyond the plaintext, or one touching a bad chunk, fails with a message and no output file; a range beside a bad chunk
succeeds; the usage errors.  The -d case (marked gpu) holds the two modes to each other byte for byte."""
import pytest

import sz_cases as sz
import sz_ranges_cases as cases
from test_cli import cli, run  # noqa: F401  (the module's fixture and helper)


def extract(cli, src, out, off, n, *mode):
    if out.exists():
        out.unlink()
    return run(cli, *mode, "-z", "-x", "%d:%d" % (off, n), "-i", str(src), "-o", str(out))


def test_cli_sz_x_host_extracts_the_slice(cli, tmp_path):
    for name, (s, plain) in cases.streams().items():
        src, out = tmp_path / (name + ".sz"), tmp_path / (name + ".out")
        src.write_bytes(s)
        for off, n in cases.edge_ranges(s, seed=3, many=3):
            r = extract(cli, src, out, off, n)
            assert r.returncode == 0 and out.read_bytes() == plain[off:off + n], (name, off, n, r.stderr)
        total = len(plain)
        for off, n in ((total, 1), (0, total + 1), (total + 1, 0), (2 ** 64 - 1, 2)):
            r = extract(cli, src, out, off, n)
            assert r.returncode != 0 and r.stderr.strip() and not out.exists(), (name, off, n)


def test_cli_sz_x_host_judges_only_the_touched_chunks(cli, tmp_path):
    for name, s in cases.parsing_damage().items():
        src, out = tmp_path / (name + ".sz"), tmp_path / (name + ".out")
        src.write_bytes(s)
        for off, n in cases.damage_ranges(s):
            st, bad, want = cases.range_model(s, off, n)
            r = extract(cli, src, out, off, n)
            if st == cases.OK:
                assert r.returncode == 0 and out.read_bytes() == want, (name, off, n, r.stderr)
            else:
                assert r.returncode != 0 and not out.exists() and ("data chunk %d " % bad) in r.stderr, (name, off, n, r.stderr)
    # a chain broken BEHIND the range's last chunk is never reached; one broken in front of its end is refused
    damaged = sz.damaged_streams()
    s = damaged["truncated_by_1"]
    src, out = tmp_path / "t.sz", tmp_path / "t.out"
    src.write_bytes(s)
    r = extract(cli, src, out, 100, 5000)
    assert r.returncode == 0 and len(out.read_bytes()) == 5000
    good = cases.chain(damaged["crc_word_bit_chunk0"])[2]       # (the same chain with its last byte: the cut took the last chunk's)
    r = extract(cli, src, out, good - 10, 10)
    assert r.returncode != 0 and not out.exists() and r.stderr.strip()
    src.write_bytes(damaged["reserved_unskippable_02"])
    assert extract(cli, src, out, 0, 9000).returncode == 0 and extract(cli, src, out, 0, 9001).returncode != 0 and not out.exists()


@pytest.mark.parametrize("extra", [("-c",), ("-T",), ("-R",), ("-S",), ("-W",), ("-r", "0:4")])
def test_cli_sz_x_usage_errors(cli, tmp_path, extra):
    src, out = tmp_path / "in.sz", tmp_path / "o"
    src.write_bytes(cases.streams()["mixed_4k"][0])
    r = run(cli, "-z", "-x", "0:4", *extra, "-i", str(src)) if "-T" in extra else run(cli, "-z", "-x", "0:4", *extra, "-i", str(src), "-o", str(out))
    assert r.returncode not in (0, 1) and r.stderr.strip() and not out.exists(), extra


def test_cli_sz_x_wants_z_and_a_well_formed_range(cli, tmp_path):
    src, out = tmp_path / "in.sz", tmp_path / "o"
    src.write_bytes(cases.streams()["mixed_4k"][0])
    r = run(cli, "-x", "0:4", "-i", str(src), "-o", str(out))
    assert r.returncode not in (0, 1) and "-z" in r.stderr and not out.exists()
    for arg in ("4", "4:", ":4", "-1:4", "1:-4", "1:4x", "a:b"):
        r = run(cli, "-z", "-x", arg, "-i", str(src), "-o", str(out))
        assert r.returncode not in (0, 1) and r.stderr.strip() and not out.exists(), arg
    assert "-x" in run(cli).stderr and "<offset>:<length>" in run(cli).stderr          # the usage text


# ---- -d: the GPU mode ----
@pytest.mark.gpu
def test_cli_sz_x_gpu_and_host_modes_write_the_same_bytes(cli, tmp_path):
    s, plain = cases.streams()["both_types_65536"]
    src, a, b = tmp_path / "in.sz", tmp_path / "a", tmp_path / "b"
    src.write_bytes(s)
    for off, n in [(0, 0), (0, 1), (65535, 2), (60000, 80000), (len(plain) - 1, 1), (0, len(plain))]:
        r = extract(cli, src, a, off, n, "-d")
        assert r.returncode == 0, (off, n, r.stderr)
        assert extract(cli, src, b, off, n).returncode == 0
        assert a.read_bytes() == b.read_bytes() == plain[off:off + n], (off, n)
    assert extract(cli, src, a, len(plain), 1, "-d").returncode != 0 and not a.exists()
    bent = sz.damaged_streams()["crc_word_bit_chunk2"]
    src.write_bytes(bent)
    assert extract(cli, src, a, 0, 9000, "-d").returncode == 0 and a.read_bytes() == cases.range_model(bent, 0, 9000)[2]
    r = extract(cli, src, a, 25000, 10, "-d")
    assert r.returncode != 0 and not a.exists() and "data chunk 2 " in r.stderr, r.stderr
