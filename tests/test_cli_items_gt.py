"""dpu_snappy -d -c -R -G and -d -c -z -G: one raw Snappy or .sz stream compressed through the calls that take a table workspace
(snappy_compress_raw_tables_gpu / snappy_compress_sz_tables_gpu).  The file written is byte for byte the one without -G, which
is the host mode's, which is the oracle's: the host-mode half of that chain runs without a GPU, and so do the usage errors."""
import pytest

import raw_cases as rc
import sz_cases as sz
from test_cli import cli, run  # noqa: F401  (the module's fixture and helper)

USAGE = 254                    # the status of every refused combination of flags (main returns -2)
BS = 4096


def _plain():
    return sz.text_random_mix(300000, 8)


def _want(fmt, plain, bs):
    import oracle_lib as oracle
    return rc.trs.convert(oracle.compress(plain, bs)) if fmt == "-R" else sz.write_sz_oracle(plain, bs)


@pytest.mark.parametrize("fmt", ["-R", "-z"])
def test_cli_host_mode_writes_the_oracles_bytes(cli, tmp_path, fmt):
    """what the -G files are compared with on the GPU, held to the oracle here"""
    plain = _plain()
    src, out = tmp_path / "in", tmp_path / "host"
    src.write_bytes(plain)
    r = run(cli, "-c", fmt, "-b", str(BS), "-i", str(src), "-o", str(out))
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == _want(fmt, plain, BS)


@pytest.mark.parametrize("flags", [("-G",), ("-G", "-c"), ("-G", "-d"), ("-G", "-d", "-c"), ("-G", "-c", "-R"), ("-G", "-c", "-z"), ("-G", "-d", "-R"),
                                   ("-G", "-d", "-z"), ("-G", "-d", "-c", "-R", "-z"), ("-G", "-d", "-c", "-z", "-T")])
def test_cli_G_without_d_c_and_one_format_is_a_usage_error(cli, tmp_path, flags):
    src, out = tmp_path / "in", tmp_path / "o"
    src.write_bytes(b"some bytes " * 10)
    r = run(cli, *flags, "-i", str(src), "-o", str(out))
    assert r.returncode == USAGE and r.stderr.strip(), (flags, r.returncode, r.stderr)
    assert not out.exists()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["-R", "-z"])
def test_cli_G_writes_the_file_of_the_host_mode_and_of_the_call_without_G(cli, tmp_path, fmt):
    plain = _plain()
    src = tmp_path / "in"
    src.write_bytes(plain)
    host, gpu, tables = tmp_path / "host", tmp_path / "gpu", tmp_path / "tables"
    assert run(cli, "-c", fmt, "-b", str(BS), "-i", str(src), "-o", str(host)).returncode == 0
    assert run(cli, "-d", "-c", fmt, "-b", str(BS), "-i", str(src), "-o", str(gpu)).returncode == 0
    r = run(cli, "-d", "-c", fmt, "-G", "-b", str(BS), "-i", str(src), "-o", str(tables))
    assert r.returncode == 0, r.stderr
    assert tables.read_bytes() == gpu.read_bytes() == host.read_bytes() == _want(fmt, plain, BS)
    back = tmp_path / "back"
    assert run(cli, fmt, "-i", str(tables), "-o", str(back)).returncode == 0 and back.read_bytes() == plain


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["raw", "sz"])
def test_drop_in_tables_functions_give_the_base_functions_bytes(fmt):
    import __graft_entry__ as entry
    entry.build_hip()
    import snappy_hip_binding as shb
    for plain, bs in ((_plain(), 32768), (_plain()[:70001], 1000), (b"", 4096), (b"x", 64)):
        base, tables = (shb.raw_compress_host, shb.raw_compress_tables_host) if fmt == "raw" else (shb.sz_compress_host, shb.sz_compress_tables_host)
        st0, want, _ = base(plain, bs)
        st1, got, rt = tables(plain, bs)
        assert (st0, st1) == (shb.SNAPPY_OK, shb.SNAPPY_OK)
        assert got == want == _want("-R" if fmt == "raw" else "-z", plain, bs), (fmt, len(plain), bs)
        assert rt["run"] > 0
    st, got, _ = (shb.raw_compress_tables_host if fmt == "raw" else shb.sz_compress_tables_host)(b"abc", 0)
    assert st != shb.SNAPPY_OK and got == b""                            # a bad block size is refused as the base function refuses it
