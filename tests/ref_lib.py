"""The reference's own host codec, run through its command line (oracle/_ref/dpu_snappy_ref, built by `make -C oracle ref`
from a reference checkout that is read in place and never copied).  Test infrastructure only.  The binary is optional:
tests that need it ask available() first; the recorded fixture (tests/golden/reference_digests.json) serves every machine
that has none."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "oracle", "_ref", "dpu_snappy_ref")
MAKE_TARGET = "make -C oracle ref REFERENCE_DIR=<reference checkout>"

MAX_FILE_LENGTH = 30 * 1024 * 1024     # dpu_snappy.h:18  #define MAX_FILE_LENGTH MEGABYTE(30)


def available():
    return os.access(BINARY, os.X_OK)


def in_reference_domain(n, stream_len):
    """Whether the reference's output for an input of n bytes is DEFINED when the framed stream takes stream_len bytes.
    snappy_compress.c:55-57 (snappy_max_compressed_length: 32 + n + n / 6, and 0 for n == 0) sizes the one buffer that
    snappy_compress.c:446-447 (setup_compression) mallocs for the whole stream, per-block size words included; nothing grows
    it, so a longer stream is written past the allocation.  dpu_snappy.h:18 caps a file at 30 MiB."""
    return stream_len <= 32 + n + n // 6 and n <= MAX_FILE_LENGTH


def _run(args, data, timeout):
    with tempfile.TemporaryDirectory(prefix="refcodec_") as d:
        src, dst = os.path.join(d, "in"), os.path.join(d, "out")
        with open(src, "wb") as f:
            f.write(data)
        # MALLOC_PERTURB_: what the reference leaves unwritten, or reads before writing, on a damaged stream is then the
        # same byte on every machine; inside the domain above nothing depends on it
        env = dict(os.environ, MALLOC_PERTURB_="90")
        try:
            p = subprocess.run([BINARY] + args + ["-i", src, "-o", dst], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                               env=env, cwd=d, timeout=timeout)
        except subprocess.TimeoutExpired:
            return -9, None
        if p.returncode != 0 or not os.path.exists(dst):
            return (p.returncode if p.returncode != 0 else 1), None
        with open(dst, "rb") as f:
            return 0, f.read()


def compress(data, block_size, timeout=120):
    """-> (exit status, framed stream or None).  A negative status is the signal that ended the binary."""
    return _run(["-c", "-b", str(block_size)], data, timeout)


def decompress(stream, timeout=120):
    """-> (exit status, plaintext or None).  255 is the reference's own rejection (main returns -1)."""
    return _run([], stream, timeout)
