"""The host-mode .sz codec of host/snappy_host.c (dpu_snappy -z without -d) under AddressSanitizer and
UndefinedBehaviorSanitizer, in a small stand-alone program of its own (nothing is loaded into Python): its chunk parser reads
hostile input.  The program holds its input in a heap block of exactly its size, so a read beyond it is reported, and is run on
the intact and on every damaged stream of tests/sz_cases.py; a sanitizer report ends it with a non-zero status that is neither
of the two the program itself returns."""
import os
import subprocess

import pytest

import sz_cases as sz
from conftest import ROOT

HOST = os.path.join(ROOT, "pim-compression_amd", "host")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]

MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include "snappy_host.h"
static int slurp(const char *path, struct host_buffer_context *c) {
    FILE *f = fopen(path, "rb"); if (!f) return 1;
    fseek(f, 0, SEEK_END); long n = ftell(f); rewind(f);
    c->buffer = malloc(n ? n : 1); c->curr = c->buffer; c->length = (unsigned long)n; c->max = ULONG_MAX;   /* exactly n bytes */
    int bad = n && fread(c->buffer, 1, n, f) != (size_t)n; fclose(f); return bad;
}
/* usage: sz d <in.sz> <out> <no_verify> | sz c <in> <out> <chunk_len>  ->  exit 0 and the result in <out>, or exit 10 + status */
int main(int argc, char **argv) {
    if (argc < 5) return 2;
    struct host_buffer_context in = { 0 }, out = { 0 };
    out.max = ULONG_MAX;
    if (slurp(argv[2], &in)) return 2;
    snappy_status st = argv[1][0] == 'c' ? snappy_compress_sz_host(&in, &out, (uint32_t)atoi(argv[4]))
                                         : snappy_decompress_sz_host(&in, &out, atoi(argv[4]));
    if (st == SNAPPY_OK) {
        FILE *f = fopen(argv[3], "wb"); if (!f) return 2;
        fwrite(out.buffer, 1, out.length, f); fclose(f);
    }
    free(out.buffer);
    free(in.buffer);
    return st == SNAPPY_OK ? 0 : 10 + (int)st;
}
'''


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("sz_sanitized")
    (d / "main.c").write_text(MAIN)
    exe = d / "sz"
    subprocess.check_call(["gcc", "--std=gnu99", "-Wall"] + SANITIZE + ["-I" + HOST, str(d / "main.c"), os.path.join(HOST, "snappy_host.c"), "-o", str(exe)])
    return str(exe)


def run(prog, *args):
    return subprocess.run([prog, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


def test_sanitized_host_parser_on_intact_and_damaged_streams(prog, tmp_path):
    for name, (s, plain) in sz.intact_streams().items():
        src, out = tmp_path / (name + ".sz"), tmp_path / (name + ".out")
        src.write_bytes(s)
        r = run(prog, "d", src, out, 0)
        assert r.returncode == 0 and out.read_bytes() == plain, (name, r.returncode, r.stderr[-1500:])
    for name, s in sz.damaged_streams().items():
        src, out = tmp_path / (name + ".sz"), tmp_path / (name + ".out")
        src.write_bytes(s)
        for no_verify in (0, 1):
            want = sz.read_sz(s, verify=not no_verify)[0]
            r = run(prog, "d", src, out, no_verify)
            assert r.returncode == (0 if want == sz.OK else 11), (name, no_verify, r.returncode, r.stderr[-1500:])    # 11: SNAPPY_INVALID_INPUT
            if want == sz.OK:
                assert out.read_bytes() == sz.read_sz(s, verify=False)[2], name
                out.unlink()
            else:
                assert not out.exists(), name
    # every prefix of a stream with all chunk kinds: truncation anywhere is refused or, at a chunk boundary, a shorter plaintext
    s = sz.intact_streams()["padding_and_skippable"][0]
    for cut in list(range(0, 40)) + list(range(len(s) - 40, len(s))):
        src = tmp_path / "cut.sz"
        src.write_bytes(s[:cut])
        want = sz.read_sz(s[:cut])[0]
        r = run(prog, "d", src, tmp_path / "cut.out", 0)
        assert r.returncode == (0 if want == sz.OK else 11), (cut, r.returncode, r.stderr[-1500:])


def test_sanitized_host_writer_is_the_model_writer(prog, tmp_path):
    for k, (plain, chunk_len) in enumerate(((sz.text_random_mix(100000, 12), 4096), (sz.text_random_mix(65537, 13), 65535), (b"", 64), (b"ab", 64),
                                            (bytes(70000), 1000))):
        src, out, back = tmp_path / ("in%d" % k), tmp_path / ("o%d.sz" % k), tmp_path / ("b%d" % k)
        src.write_bytes(plain)
        r = run(prog, "c", src, out, chunk_len)
        assert r.returncode == 0, (k, r.stderr[-1500:])
        assert out.read_bytes() == sz.write_sz_oracle(plain, chunk_len), k
        assert run(prog, "d", out, back, 0).returncode == 0 and back.read_bytes() == plain, k
    assert run(prog, "c", src, out, 63).returncode == 11 and run(prog, "c", src, out, 65536).returncode == 11
