"""The constructed K1 inputs -- the strided-scan ones (tests/k1_strided_cases.py) and the alias ones (tests/k1_alias_cases.py) --
as calls of the four kernels that carry K1's parse besides the two product kernels (csrc/snappy_kernels.hpp:
LDS_TABLE_WAVE_COMPRESS): update (recompress_dirty_kernel), resize (resize_recompress_kernel), raw
(raw_compress_fragments_kernel) and .sz (sz_compress_chunks_kernel).  tests/test_k1_carriers_emulated.py sends these calls
through the wave emulator and tests/test_gpu_k1_carriers.py through the C ABI; both take the calls and the bytes each must
give from here, and every expected byte comes from the oracle.  A new K1 edge case is added once, to inputs()."""
import functools

import k1_alias_cases
import k1_strided_cases
import oracle_lib as oracle
import ranges_cases as rc
import raw_cases
import resize_cases as rz
import sz_cases as sz
import update_cases as uc
from conftest import golden_bytes

FORMS = (3, 2)                      # K1's parse: 3 = the stream form, 2 = the bulk form
PRODUCT_VARIANT = {3: 3501, 2: 2501}  # the product's LDS-table kernel in the same form (tests/test_emulated_kernels.py)


@functools.lru_cache(maxsize=None)
def inputs():
    """((name, data, block size), ...): the strided-scan inputs, then the alias inputs as alias/<name>"""
    return tuple(k1_strided_cases.cases()) + tuple(("alias/" + name, data, bs) for name, data, bs in k1_alias_cases.cases())


def is_alias(name):
    return name.startswith("alias/")


def is_built(name):
    """the alias inputs whose every window was constructed: the stream form must take them"""
    return name.startswith("alias/built/")


def spare(i):
    """bytes in front of the source of input (or write, or segment) i on the device: sources at every alignment"""
    return i % 16 + 1


@functools.lru_cache(maxsize=None)
def groups():
    """((block size, (index into inputs(), ...)), ...): the inputs of one block size are the items of ONE raw or .sz call"""
    by_bs = {}
    for i, (_, _, bs) in enumerate(inputs()):
        by_bs.setdefault(bs, []).append(i)
    return tuple((bs, tuple(idx)) for bs, idx in by_bs.items())


class BatchCall:
    """One raw or .sz compress call: block_size (chunk_len), the indexes into inputs() of its items, wants [expected stream],
    caps [capacity], items [(plaintext, capacity)], max_units (fragments or chunks of all items together)."""

    def __init__(self, bs, indexes, wants, caps):
        self.block_size, self.indexes, self.wants, self.caps = bs, indexes, wants, caps
        self.names = [inputs()[i][0] for i in indexes]
        self.plains = [inputs()[i][1] for i in indexes]
        self.items = list(zip(self.plains, caps))
        self.max_units = sum(-(-len(p) // bs) for p in self.plains)

    def alone(self, k):
        """item k as a call of its own (same capacity): where statistics are wanted per input"""
        return BatchCall(self.block_size, self.indexes[k:k + 1], self.wants[k:k + 1], self.caps[k:k + 1])


def _batch_calls(want, bound):
    """one call per group; capacity: exactly the expected length for odd inputs, the interface's bound for even ones"""
    calls = []
    for bs, indexes in groups():
        wants = [want(inputs()[i][1], bs) for i in indexes]
        caps = [len(w) if i % 2 else bound(len(inputs()[i][1]), bs) for i, w in zip(indexes, wants)]
        calls.append(BatchCall(bs, indexes, wants, caps))
    return tuple(calls)


def raw_bound(n, bs):
    """snappy_hip_raw_compress_bound"""
    return 5 + -(-n // bs) * 32 + n + n // 6


def sz_bound(n, chunk_len):
    """snappy_hip_sz_compress_bound"""
    return 10 + 8 * -(-n // chunk_len) + n


@functools.lru_cache(maxsize=None)
def raw_calls():
    """block_size = the input's block size: every fragment is a block of the input, converted from the oracle's stream"""
    return _batch_calls(lambda data, bs: raw_cases.trs.convert(oracle.compress(data, bs)), raw_bound)


@functools.lru_cache(maxsize=None)
def sz_calls():
    """chunk_len = the input's block size.  A chunk is stored plain where K1's output is not shorter, and then only K1's length
    shows: sz_compressed_chunks() counts what is left."""
    return _batch_calls(sz.write_sz_oracle, sz_bound)


def sz_compressed_chunks(stream):
    """(chunks of type 0x00, data chunks) of an expected .sz stream"""
    at, compressed, data = len(sz.IDENTIFIER), 0, 0
    while at < len(stream):
        kind, n = stream[at], int.from_bytes(stream[at + 1:at + 4], "little")
        assert kind in (0, 1)
        compressed += kind == 0
        data += 1
        at += 4 + n
    assert at == len(stream)
    return compressed, data


def assert_sz_inputs_stay_visible():
    """Every alias input has only compressed chunks and the planted construction at least 4: their parse shows in the bytes.
    Should a change to the inputs lose that, the .sz tests fail instead of passing on K1's lengths alone."""
    seen = 0
    for call in sz_calls():
        for name, want in zip(call.names, call.wants):
            compressed, data = sz_compressed_chunks(want)
            if is_alias(name):
                assert compressed == data >= 1, (name, compressed, data)
                seen += 1
            elif name == "planted":
                assert compressed >= 4, (name, compressed, data)
                seen += 1
    assert seen == 7


def update_calls(data, bs):
    """[(tag, container, writes [(offset, bytes)], expected stream)]:
    (a) a container of zeros with one write of the whole input: every block is dirty and covered, none is decoded;
    (b) the input's own container with one 1-byte write per block that stores the byte already there: every block is decoded
        by K2 into the patch slot, patched and parsed again, and the new stream is the old one."""
    ref = oracle.compress(data, bs)
    own = rc.Container(data, ref)
    ats = [b * bs + b % 7 for b in range(own.num_blocks)]
    assert ats and all(at < len(data) for at in ats)
    return [("a", rc.Container(bytes(len(data)), block_size=bs), [(0, data)], ref),
            ("b", own, [(at, data[at:at + 1]) for at in ats], ref)]


def resize_calls(data, bs):
    """[(tag, container, keep_len, segments [bytes], expected stream, blocks parsed)]:
    (a) the first bs // 3 bytes as the container and the rest appended as 1 byte, half, the remainder: the cut block is decoded,
        gathered and parsed, and every block is new;
    (b) the input with 100 bytes of text behind it, truncated to the input: the last block is parsed again at its own, shorter
        length -- where the input does not end on a block boundary; where it does, nothing is parsed."""
    keep = bs // 3
    rest = data[keep:]
    half = len(rest) // 2
    nb = -(-len(data) // bs)
    return [("a", rc.Container(data[:keep], block_size=bs), keep, [rest[:1], rest[1:1 + half], rest[1 + half:]], oracle.compress(data, bs), nb),
            ("b", rc.Container(data + golden_bytes("alice.txt")[:100], block_size=bs), len(data), [], oracle.compress(data, bs), nb - len(data) // bs)]


def expected_update(c, writes, want):
    """update_cases.expected, held to the stream the case states"""
    exp = uc.expected(c, writes)
    assert exp[0] == want
    return exp


def expected_resize(c, keep_len, segments, want, parsed):
    exp = rz.expected(c, keep_len, segments)
    assert exp[0] == want and exp[2] == parsed
    return exp
