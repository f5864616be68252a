"""dpu_snappy -t KEEP_LEN and -a TAILFILE in host mode (no -d): only the block the cut falls into is decoded, only it and the
blocks behind it are compressed, and the output file is byte for byte what `dpu_snappy -c` writes for the new plaintext (and
the oracle's stream); the argument errors end with a message, a non-zero exit and no output file."""
import os

import pytest

import oracle_lib as oracle
import ranges_cases as rc
import resize_cases as rz
from conftest import GOLDEN, golden_bytes
from test_cli import LINES, check_stdout_contract, cli, run  # noqa: F401  (the module's fixture and helpers)

assert len(LINES) == 11


def _compressed_by_cli(cli, tmp_path, plain, bs):
    src, out = tmp_path / "new.txt", tmp_path / "new.snappy"
    src.write_bytes(plain)
    r = run(cli, "-c", "-b", str(bs), "-i", str(src), "-o", str(out))
    assert r.returncode == 0, r.stderr
    return out.read_bytes()


def _resize_cases(c):
    """(keep_len or None for "-a alone", tail or None for "-t alone")"""
    bs, total = c.block_size, c.total
    b = rz.boundary(total, bs) or 0
    more = rz.tail_bytes(c.plain, total, 2 * bs + 5, "random", seed=1)
    return [(total // 3, None), (b, None), (0, None), (total, None),                          # -t alone
            (None, b"x"), (None, more), (None, b""),                                          # -a alone keeps everything
            (total // 3, rz.tail_bytes(c.plain, total // 3, bs - total // 3 % bs, "zeros")),  # both: the cut block filled exactly
            (b, more), (max(b - 1, 0), c.plain[max(b - 1, 0):]), (0, b"new"), (total, more)]


@pytest.mark.parametrize("name", ["alice", "terror2", "blocks7"])
def test_cli_resize_host_matches_cli_compress_and_oracle(cli, tmp_path, name):
    """alice and terror2 (the reference's own streams) and one file of 7-byte blocks, which only the oracle writes: the host
    mode's -c takes block sizes from 64 up."""
    if name == "blocks7":
        plain = golden_bytes("coding.txt")[:1500]
        path = tmp_path / "blocks7.snappy"
        path.write_bytes(oracle.compress(plain, 7))
    else:
        plain = golden_bytes(name + ".txt")
        path = os.path.join(GOLDEN, name + ".snappy")
    c = rc.Container(plain, open(path, "rb").read())
    for k, (keep_len, tail) in enumerate(_resize_cases(c)):
        args = [] if keep_len is None else ["-t", str(keep_len)]
        if tail is not None:
            tf = tmp_path / f"{k}.tail"
            tf.write_bytes(tail)
            args += ["-a", str(tf)]
        out = tmp_path / f"{k}.out"
        r = run(cli, *args, "-i", str(path), "-o", str(out))
        assert r.returncode == 0, (args, r.stderr)
        got = out.read_bytes()
        new_plain = plain[:c.total if keep_len is None else keep_len] + (tail or b"")
        assert got == oracle.compress(new_plain, c.block_size), (keep_len, len(tail or b""))
        if c.block_size >= 64:
            assert got == _compressed_by_cli(cli, tmp_path, new_plain, c.block_size)
        if new_plain == plain:
            assert got == c.stream
        check_stdout_contract(r.stdout)
        assert f"Compressed {len(got)} bytes to: {out}" in r.stdout


@pytest.mark.parametrize("arg", ["", "x", "10x", "-1", "1:2", " 5"])
def test_cli_resize_malformed_keep_length(cli, tmp_path, arg):
    r = run(cli, "-t", arg, "-i", os.path.join(GOLDEN, "alice.snappy"), "-o", str(tmp_path / "o"))
    assert r.returncode != 0 and r.stderr.strip()
    assert not (tmp_path / "o").exists()


def test_cli_resize_with_other_modes_missing_tail_and_beyond_the_file(cli, tmp_path):
    tf = tmp_path / "tail"
    tf.write_bytes(b"0123456789")
    alice = os.path.join(GOLDEN, "alice.snappy")
    for other in (["-c"], ["-r", "0:10"], ["-w", f"0:{tf}"], ["-R"]):
        for mine in (["-t", "5"], ["-a", str(tf)]):
            r = run(cli, *other, *mine, "-i", alice, "-o", str(tmp_path / "c"))
            assert r.returncode != 0 and "-t and -a" in r.stderr, (other, mine)
            assert not (tmp_path / "c").exists()
    r = run(cli, "-a", str(tmp_path / "missing"), "-i", alice, "-o", str(tmp_path / "m"))
    assert r.returncode != 0 and r.stderr.strip()
    assert not (tmp_path / "m").exists()
    total = len(golden_bytes("alice.txt"))
    for keep in (total + 1, (1 << 64) - 1):
        r = run(cli, "-t", str(keep), "-a", str(tf), "-i", alice, "-o", str(tmp_path / "b"))
        assert r.returncode != 0 and r.stderr.strip(), keep
        assert not (tmp_path / "b").exists()
    # a damaged container: the chain does not end at the file's end; a header that cannot be read
    bad = tmp_path / "bad.snappy"
    bad.write_bytes(golden_bytes("terror2.snappy")[:-5])
    for args in (["-t", "0"], ["-a", str(tf)]):
        r = run(cli, *args, "-i", str(bad), "-o", str(tmp_path / "d"))
        assert r.returncode != 0 and "Encountered Snappy error" in r.stderr
        assert not (tmp_path / "d").exists()
    bad.write_bytes(b"\xff\xff\xff\xff\xff\xff")
    r = run(cli, "-a", str(tf), "-i", str(bad), "-o", str(tmp_path / "h"))
    assert r.returncode != 0 and r.stderr.strip() and not (tmp_path / "h").exists()
    usage = run(cli).stderr                                    # the usage line names both
    assert "-t <keep_len>" in usage and "-a <tail_file>" in usage
