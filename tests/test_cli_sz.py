"""dpu_snappy -z: the Snappy framing format (.sz).  Host mode (no -d): -c -z writes exactly the model writer's bytes over the
oracle's blocks, -z reads the model's and pyarrow-made streams and refuses every damaged one, -z -T verifies by decoding and
exits 0 or 1.  The -d cases (marked gpu) hold the two modes to each other byte for byte, each reading what the other wrote."""
import os
import re

import pytest

import datagen
import sz_cases as sz
from conftest import GOLDEN, golden_bytes
from test_cli import LINES, check_stdout_contract, cli, run  # noqa: F401  (the module's fixture and helpers)


@pytest.mark.parametrize("bs", [64, 4096, 65535])
@pytest.mark.parametrize("name", ["terror2", "coding"])
def test_cli_sz_host_compress_is_the_model_writer_and_round_trips(cli, tmp_path, name, bs):
    src = os.path.join(GOLDEN, name + ".txt")
    plain = golden_bytes(name + ".txt")
    out, back = tmp_path / "o.sz", tmp_path / "back"
    r = run(cli, "-c", "-z", "-b", str(bs), "-i", src, "-o", str(out))
    assert r.returncode == 0, r.stderr
    check_stdout_contract(r.stdout)
    got = out.read_bytes()
    assert got == sz.write_sz_oracle(plain, bs)
    st, n, decoded, _ = sz.read_sz(got)
    assert (st, n) == (sz.OK, len(plain)) and decoded == plain
    r = run(cli, "-z", "-i", str(out), "-o", str(back))
    assert r.returncode == 0, r.stderr
    check_stdout_contract(r.stdout)
    assert back.read_bytes() == plain
    r = run(cli, "-z", "-T", "-i", str(out))
    assert r.returncode == 0 and re.search(r"^Check: OK, %d bytes$" % len(plain), r.stdout, re.M), r.stdout


def test_cli_sz_host_mixed_and_random_and_empty_input(cli, tmp_path):
    for k, plain in enumerate((sz.text_random_mix(150000, 4), datagen.random_bytes(70000, seed=4), b"", b"x")):
        src, out, back = tmp_path / ("in%d" % k), tmp_path / ("o%d.sz" % k), tmp_path / ("back%d" % k)
        src.write_bytes(plain)
        assert run(cli, "-c", "-z", "-b", "1000", "-i", str(src), "-o", str(out)).returncode == 0
        got = out.read_bytes()
        assert got == sz.write_sz_oracle(plain, 1000)
        if k == 1:
            assert len(got) == 10 + 8 * 70 + 70000          # random bytes: every chunk uncompressed, the bound exactly
        if k == 2:
            assert got == sz.IDENTIFIER
        assert run(cli, "-z", "-i", str(out), "-o", str(back)).returncode == 0 and back.read_bytes() == plain


def test_cli_sz_host_reads_third_party_and_odd_streams(cli, tmp_path):
    for name, (s, plain) in sz.intact_streams().items():
        src, out = tmp_path / (name + ".sz"), tmp_path / (name + ".out")
        src.write_bytes(s)
        r = run(cli, "-z", "-i", str(src), "-o", str(out))
        assert r.returncode == 0, (name, r.stderr)
        assert out.read_bytes() == plain, name
        assert run(cli, "-z", "-T", "-i", str(src)).returncode == 0, name


def test_cli_sz_host_refuses_damaged_streams(cli, tmp_path):
    for name, s in sz.damaged_streams().items():
        assert sz.read_sz(s)[0] != sz.OK
        src, out = tmp_path / (name + ".sz"), tmp_path / (name + ".out")
        src.write_bytes(s)
        r = run(cli, "-z", "-i", str(src), "-o", str(out))
        assert r.returncode != 0 and not out.exists() and r.stderr.strip(), name
        r = run(cli, "-z", "-T", "-i", str(src))
        assert r.returncode == 1 and re.search(r"^Check: INVALID$", r.stdout, re.M), (name, r.returncode, r.stdout)


@pytest.mark.parametrize("extra", [("-R",), ("-r", "0:10"), ("-t", "5"), ("-W",), ("-T", "-c"), ("-T", "-o", "OUT")])
def test_cli_sz_usage_errors(cli, tmp_path, extra):
    src = tmp_path / "in.sz"
    src.write_bytes(sz.IDENTIFIER)
    args = [str(tmp_path / "o2") if a == "OUT" else a for a in extra]
    r = run(cli, "-z", *args, "-i", str(src), "-o", str(tmp_path / "o")) if "-T" not in extra else run(cli, "-z", *args, "-i", str(src))
    assert r.returncode not in (0, 1) and r.stderr.strip()
    assert not (tmp_path / "o").exists() and not (tmp_path / "o2").exists()


def test_cli_sz_host_bad_chunk_len(cli, tmp_path):
    for bs in ("0", "63", "65536"):
        r = run(cli, "-c", "-z", "-b", bs, "-i", os.path.join(GOLDEN, "coding.txt"), "-o", str(tmp_path / "o"))
        assert r.returncode != 0 and not (tmp_path / "o").exists(), bs


# ---- -d: the GPU mode ----
@pytest.mark.gpu
@pytest.mark.parametrize("bs", [4096, 65535])
def test_cli_sz_gpu_and_host_modes_write_the_same_bytes_and_read_each_other(cli, tmp_path, bs):
    plain = sz.text_random_mix(300000, 8)
    src = tmp_path / "in"
    src.write_bytes(plain)
    host_sz, gpu_sz = tmp_path / "host.sz", tmp_path / "gpu.sz"
    assert run(cli, "-c", "-z", "-b", str(bs), "-i", str(src), "-o", str(host_sz)).returncode == 0
    r = run(cli, "-d", "-c", "-z", "-b", str(bs), "-i", str(src), "-o", str(gpu_sz))
    assert r.returncode == 0, r.stderr
    check_stdout_contract(r.stdout, gpu=False)
    assert gpu_sz.read_bytes() == host_sz.read_bytes() == sz.write_sz_oracle(plain, bs)
    assert sz.read_sz(gpu_sz.read_bytes())[2] == plain
    a, b = tmp_path / "a", tmp_path / "b"
    r = run(cli, "-d", "-z", "-i", str(host_sz), "-o", str(a))             # the GPU reads what the host wrote
    assert r.returncode == 0 and a.read_bytes() == plain, r.stderr
    assert run(cli, "-z", "-i", str(gpu_sz), "-o", str(b)).returncode == 0 and b.read_bytes() == plain
    assert run(cli, "-d", "-z", "-T", "-i", str(gpu_sz)).returncode == 0


@pytest.mark.gpu
def test_cli_sz_gpu_reads_third_party_streams_and_refuses_damaged_ones(cli, tmp_path):
    s, plain = sz.intact_streams()["pyarrow_65536"]
    src, out = tmp_path / "p.sz", tmp_path / "p.out"
    src.write_bytes(s)
    r = run(cli, "-d", "-z", "-i", str(src), "-o", str(out))
    assert r.returncode == 0 and out.read_bytes() == plain, r.stderr
    damaged = sz.damaged_streams()
    for name in ("crc_word_bit_chunk2", "payload_bit_compressed", "reserved_unskippable_02", "truncated_by_1", "varint_says_65537", "elements_damaged"):
        src, out = tmp_path / (name + ".sz"), tmp_path / (name + ".out")
        src.write_bytes(damaged[name])
        r = run(cli, "-d", "-z", "-i", str(src), "-o", str(out))
        assert r.returncode != 0 and not out.exists(), name
        assert run(cli, "-d", "-z", "-T", "-i", str(src)).returncode == 1, name
