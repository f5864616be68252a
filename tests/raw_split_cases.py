"""Cases of the split decode of raw Snappy streams (snappy_hip_raw_decompress_split_batch), shared by the
emulator and the GPU tests, and a MODEL of its steps 2-4 in plain Python.

The call's proof sits in its step 5, so a mistake in the segment walk, the resolve or the cuts still gives the right bytes and
the right status: the item merely falls back to the serial decoder.  Only the four result words can show that.  model() says
what they must be for any VALID stream -- one serial walk over the elements that shares no code with the kernels -- and what
the cut table and the resolve step's nodes must hold.  The generators below write what no greedy compressor writes; the
coverage conditions are computed from the model alone, so the inputs cannot quietly stop covering a case."""
import numpy as np

import datagen
import raw_cases as rc

NONE = 0xffffffff
ZONE = 64
KINDS = ("literal_0", "literal_1", "literal_2", "literal_3", "literal_4", "copy_1", "copy_2", "copy_4")
SPLIT, SMALL, FELL_BACK = [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]


# ---- the model ----
def elements(stream, at):
    """the elements of stream[at:] as (position, kind, compressed bytes, output bytes, copy offset or None); the walk ends at
    the first element that does not fit the stream -> (elements, True if it reached the stream's end exactly)"""
    out, n = [], len(stream)
    while at < n:
        tag = stream[at]
        t, v = tag & 3, tag >> 2
        if t == 0:
            nb = v - 59 if v >= 60 else 0
            if at + 1 + nb > n:
                return out, False
            olen = (int.from_bytes(stream[at + 1:at + 1 + nb], "little") if nb else v) + 1
            size, kind, off = 1 + nb + olen, nb, None
            if olen > 0xffffffff:
                return out, False
        else:
            hdr = (2, 3, 5)[t - 1]
            if at + hdr > n:
                return out, False
            olen = (v & 7) + 4 if t == 1 else v + 1
            off = ((tag >> 5) << 8) | stream[at + 1] if t == 1 else int.from_bytes(stream[at + 1:at + hdr], "little")
            size, kind = hdr, 4 + t
        if at + size > n:
            return out, False
        out.append((at, kind, size, olen, off))
        at += size
    return out, True


class Model:
    pass


def model(stream, unit_len, segment_bytes):
    """What steps 1-4 must make of one stream whose header parses.  For a valid stream: cuts (units + 1 of them, NONE where no
    element starts at k * unit_len, the last one src_len), independent, split_class, words, nodes (segment -> (entry, landing,
    output base) for every segment the true chain enters), and for coverage entry_offsets (segment -> entry - segment start),
    passed (segments the chain passes by), straddlers (segment -> kind of the element across its start) and unit_starts
    (unit -> kind).  For a stream whose chain breaks (valid False) the nodes are those in front of the break, no cut exists."""
    m = Model()
    m.length, m.hdr = rc.header_parses(stream)
    m.src_len = n = len(stream)
    els, m.valid = elements(stream, m.hdr)
    m.units = -(-m.length // unit_len)
    m.segments = -(-(n - m.hdr) // segment_bytes)
    m.split_class = m.length > unit_len and m.segments > 1
    m.cuts = [NONE] * (m.units + 1)
    m.independent = True
    m.unit_starts, m.entry_offsets, m.straddlers, m.nodes = {}, {}, {}, {}
    op = 0
    first = {}                                           # segment -> index of the first element that starts in it
    base = []
    for k, (pos, kind, size, olen, off) in enumerate(els):
        base.append(op)
        if op % unit_len == 0 and op // unit_len < m.units:
            m.cuts[op // unit_len] = pos
            m.unit_starts[op // unit_len] = kind
        if off is not None and off > op % unit_len:
            m.independent = False
        first.setdefault((pos - m.hdr) // segment_bytes, k)
        op += olen
    m.valid = m.valid and op == m.length
    starts = [e[0] for e in els] + [els[-1][0] + els[-1][2] if els else m.hdr]      # (the last: src_len, or where the chain breaks)
    for s, k in sorted(first.items()):
        zone = m.hdr + s * segment_bytes
        end = min(zone + segment_bytes, n)
        j = next((j for j in range(k, len(starts)) if starts[j] >= end), None)
        if j is None:
            break                                        # the chain breaks inside this segment: no node for it or behind it
        m.nodes[s] = (els[k][0], starts[j], base[k])
        m.entry_offsets[s] = els[k][0] - zone
        if s and els[k][0] > zone:
            m.straddlers[s] = els[k - 1][1]
    m.passed = [s for s in range(m.segments) if s not in first]
    if m.valid:
        m.cuts[m.units] = n
        m.words = SMALL if not m.split_class else (SPLIT if m.independent and NONE not in m.cuts else FELL_BACK)
    else:
        m.cuts = [NONE] * (m.units + 1)
        m.words = None
    return m


def batch_words(models, max_segments=None, max_units=None):
    """the four result words of one call over valid items: the sum of the models' words, with every split-class item from
    the first one that does not fit the limits on handed to the serial decoder, as the plan does it"""
    words = [0, 0, 0, 0]
    segs = units = 0
    for m in models:
        w = m.words
        if m.split_class:
            segs += m.segments
            units += m.units
            if (max_segments is not None and segs > max_segments) or (max_units is not None and units > max_units):
                w = FELL_BACK
        words = [a + b for a, b in zip(words, w)]
    return words


# ---- streams that no greedy compressor writes ----
def padded_header(n, header_bytes):
    v = bytearray(rc.varint(n))
    assert len(v) <= header_bytes <= 5
    if len(v) < header_bytes:
        v[-1] |= 0x80
        v += bytes([0x80]) * (header_bytes - len(v) - 1) + b"\x00"
    return bytes(v)


def fragment_stream(total, fragment, seed, flavour, header_bytes=None):
    """(stream, plaintext): datagen.element_stream's blocks as one raw stream -- literals with 0-4 length bytes (non-minimal
    too), copies of 1-64 with 1-, 2- and 4-byte offsets, dependent chains -- fragment-built by construction.  header_bytes pads
    the length varint, which shifts every segment start against the elements."""
    framed, plain = datagen.element_stream(total, fragment, seed, flavour)
    s = rc.trs.convert(framed)
    if header_bytes is not None:
        s = padded_header(total, header_bytes) + s[rc.header_parses(s)[1]:]
    return s, plain


def raw_element_stream(total, seed, flavour):
    """(stream, plaintext) of what only the raw format allows: copies that reach back across any boundary (COPY_2 up to 65,535,
    COPY_4 beyond 65,536), literals of up to about 100,000 bytes, 3- and 4-byte length fields on short literals.  flavour 0:
    short elements of every kind; 1: long literals between them; 2: literals only just longer than a zone.  The plaintext
    comes from tools/to_raw_snappy.decode_raw."""
    r = np.random.default_rng(seed)
    parts, op = [], 0
    while op < total:
        left = total - op
        c = r.random()
        if op == 0 or c < (0.45, 0.5, 0.6)[flavour]:
            if flavour == 1 and r.random() < 0.08:
                ln = int(r.choice([300, 1000, 5000, 20000, 100000]))
            elif flavour == 2:
                ln = int(r.integers(56, 140))
            else:
                ln = int(r.integers(1, 72))
            ln = min(ln, left)
            least = 0 if ln <= 60 else (ln - 1).bit_length() + 7 >> 3
            nb = int(r.integers(max(least, 1), 5)) if r.random() < 0.6 else least
            parts.append(rc.literal(r.integers(0, 256, size=ln, dtype=np.uint8).tobytes(), nb or None))
        else:
            ln = min(int(r.choice([1, 2, 3, 4, 5, 8, 11, 12, 33, 64])), left)
            c = r.random()
            if c < 0.3:
                off = int(r.integers(1, min(op, 64) + 1))
            elif c < 0.6:
                off = int(r.integers(1, min(op, 65535) + 1))
            elif c < 0.8:
                off = min(op, 65535)
            else:
                off = int(r.integers(max(1, op - op // 8), op + 1))             # far back, beyond 65,536 once there is that much
            c = r.random()
            if 4 <= ln <= 11 and off < 2048 and c < 0.4:
                parts.append(rc.copy1(ln, off))
            elif off < 65536 and c < 0.8:
                parts.append(rc.copy2(ln, off))
            else:
                parts.append(rc.copy4(ln, off))
        op += ln
    s = rc.varint(total) + b"".join(parts)
    return s, rc.trs.decode_raw(s)


# ---- hand-built stream ends (unit_len 256, segments of 128 bytes, headers of 2 bytes) ----
def _literals(sizes, seed):
    data = datagen.random_bytes(sum(sizes), seed=seed)
    out, at = [], 0
    for n in sizes:
        out.append(rc.literal(data[at:at + n]))
        at += n
    return out


def stream_ends():
    """name -> (valid stream, the same cut short by one byte).  The last element is the one whose tag lies 1 to 7 bytes in
    front of src_len, where an element's size is gathered byte by byte; every kind is there, the literals with 1-4 length bytes
    so that the header ends on the stream's last bytes.  Three units of 60-byte literals lead up to it: the last segment is
    entered in its zone, so the table entry looked up for it and the lanes of the last segment's walk end on that element."""
    unit = [60, 60, 60, 60, 16]
    r = datagen.random_bytes
    ends = {"literal_0_1": (rc.literal(b"a"), 1), "literal_0_6": (rc.literal(r(6, seed=51)), 6), "copy_1": (rc.copy1(4, 9), 4),
            "copy_2": (rc.copy2(1, 200), 1), "copy_4": (rc.copy4(3, 130), 3)}
    for nb in (1, 2, 3, 4):
        ends["literal_%d_1" % nb] = (rc.literal(b"z", nb), 1)
        ends["literal_%d_2" % nb] = (rc.literal(b"yz", nb), 2)
    v = {}
    for k, (name, (last, olen)) in enumerate(sorted(ends.items())):
        rest = 256 - olen                                  # the last unit: literals up to the last element, which ends it exactly
        sizes = unit * 2 + [60] * (rest // 60) + ([rest % 60] if rest % 60 else [])
        s = rc._sized(_literals(sizes, 60 + k) + [last])
        assert 1 <= len(last) <= 7 and rc.header_parses(s) == (768, 2) and rc.expect(s)[0] == rc.OK, name
        assert rc.expect(s[:-1])[0] == rc.INVALID, name
        v[name] = (s, s[:-1])
    return v


def copy_reach_streams():
    """name -> stream: in the second unit, 60 bytes in, a copy whose offset is exactly 60 (it reads the unit's first byte: the
    unit is its own) and one whose offset is 61 (the last byte of the unit in front: the item falls back), for every kind of copy"""
    unit = [60, 60, 60, 60, 16]
    v = {}
    for k, (name, copy) in enumerate((("copy_1", rc.copy1), ("copy_2", rc.copy2), ("copy_4", rc.copy4))):
        for off in (60, 61):
            v["%s_offset_%d" % (name, off)] = rc._sized(_literals(unit + [60], 80 + k) + [copy(8, off)] + _literals([60, 60, 60, 8] + unit, 90 + k))
    return v


def hostile_ends():
    """name -> stream, all INVALID: the last element is a literal with a 4-byte length field whose TOP byte is set -- the fifth
    byte of the element, the last one a sizing by hand may gather -- while the three bytes below it give exactly the payload
    that is there.  A sizing that drops that byte finds a well-shaped chain where there is none."""
    unit = [60, 60, 60, 60, 16]
    v = {}
    for k in (1, 2):
        payload = datagen.random_bytes(k, seed=70 + k)
        rest = 256 - k
        sizes = unit * 2 + [60] * (rest // 60) + [rest % 60]
        body = b"".join(_literals(sizes, 72 + k)) + rc.literal_field(0x01000000 | (k - 1), payload)
        s = rc.varint(768) + body
        assert rc.expect(s)[0] == rc.INVALID
        v["top_byte_set_%d" % k] = s
    return v


# ---- coverage, from the model alone ----
def coverage(models):
    c = Model()
    c.entry_offsets = set()
    c.straddlers, c.unit_starts = set(), set()
    c.passed = 0
    for m in models:
        if not (m.valid and m.split_class):
            continue
        c.entry_offsets |= set(m.entry_offsets.values())
        c.straddlers |= set(m.straddlers.values())
        c.unit_starts |= set(m.unit_starts.values())
        c.passed += len(m.passed)
    return c


def assert_covers(models):
    c = coverage(models)
    assert set(range(ZONE)) <= c.entry_offsets, sorted(set(range(ZONE)) - c.entry_offsets)      # every zone offset is an entry
    assert any(o >= ZONE for o in c.entry_offsets)                                               # resolve's walked path
    assert c.passed > 0                                                                          # a segment passed by entirely
    assert c.straddlers == set(range(8)), [KINDS[k] for k in set(range(8)) - c.straddlers]
    assert c.unit_starts == set(range(8)), [KINDS[k] for k in set(range(8)) - c.unit_starts]
    split = [m.words for m in models if m.valid and m.split_class]
    assert 4 * split.count(SPLIT) >= len(split) and 4 * split.count(FELL_BACK) >= len(split), (split.count(SPLIT), split.count(FELL_BACK))


# ---- the model-driven batches ----
CONFIGS = ((256, 128), (512, 192), (256, 320))           # (unit_len, segment_bytes) of the three calls
FRAGMENTS = (256, 384, 512, 640, 768, 1000, 1024, 1536, 2048, 4096)


def hand_streams():
    import test_raw_split_emulated as t
    return {name: s for name, (s, _) in t.hand_streams().items()}


def model_batch(config):
    """[(name, stream, plaintext)] of one call: about a hundred valid items -- fragment-built streams at fragments the unit
    divides and at fragments it does not, with headers of 1-5 bytes, raw-only streams, the hand-built streams, stream ends
    and copies to either side of a unit's first byte,
    and in the first call the third-party fixtures."""
    k = CONFIGS.index(config)
    items = []
    for j in range(60):
        # every other one at a fragment whose multiples the unit's are: these split; the rest meets unit boundaries by chance
        fragment = (config[0] if j % 4 or config[0] == 256 else config[0] // 2) if j % 2 else FRAGMENTS[(j // 2 + 3 * k) % len(FRAGMENTS)]
        total = fragment * (3 + j % 5) + (0, 1, fragment // 3)[j % 3]
        hb = max(1 + (j + k) % 5, len(rc.varint(total)))
        s, p = fragment_stream(total, fragment, 1000 * k + j, j % 4, hb)
        items.append(("fragment_%d_%d_%d" % (fragment, j, hb), s, p))
    for j in range(18):
        total = (3000, 9000, 20000, 40000)[j % 4] if j < 16 else (150000, 300000)[j - 16] if k == j - 16 else 5000
        s, p = raw_element_stream(total, 2000 * (k + 1) + j, j % 3)
        items.append(("raw_%d_%d" % (total, j), s, p))
    for name, s in hand_streams().items():
        items.append((name, s, rc.expect(s)[2]))
    for name, (s, _) in stream_ends().items():
        items.append(("end_" + name, s, rc.expect(s)[2]))
    for name, s in copy_reach_streams().items():
        items.append((name, s, rc.expect(s)[2]))
    if k == 0:
        items += [(name, rc.fixture_stream(name), rc.fixture_plain(name)) for name in rc.FIXTURES]
    return items


# ---- fragment-built streams: never a fallback ----
def fragment_built_calls():
    """[(unit_len, segment_bytes, [(stream, plaintext)])]: for fragments of 256, 1,024 and 4,096 every flavour of
    datagen.element_stream under headers of every size from the shortest the length allows to 5 bytes (a split-class item
    is longer than 127 bytes, so never 1), decoded in units of the fragment and of twice the fragment."""
    calls = []
    for k, fragment in enumerate((256, 1024, 4096)):
        items = []
        for flavour in range(4):
            total = fragment * (4 + flavour % 2) + (0, 1, fragment // 2 + 7, fragment - 1)[flavour]
            for hb in range(len(rc.varint(total)), 6):
                items.append(fragment_stream(total, fragment, 3000 + 10 * k + flavour, flavour, hb))
        calls += [(fragment, (128, 192, 320)[k], items), (2 * fragment, (128, 320, 192)[k], items)]
    return calls


# ---- more items than one trip of the planner ----
TRIP_SPLIT_AT = (3, 1023, 1024, 1030)
TRIP_COUNT = 1032


def planner_trip_items():
    """[(stream, plaintext)]: 1,032 items for units of 256 and segments of 128, tiny one-literal ones but for four split-class
    ones: the last of the plan's first trip of 1,024, the first of its second, and one deep in the second with 80 units (more
    than a 256-byte line of cut words)."""
    big = {3: fragment_stream(1024 + 100, 256, 4001, 0), 1023: fragment_stream(6 * 256, 256, 4002, 1), 1024: fragment_stream(3 * 768, 768, 4003, 0),
           1030: fragment_stream(80 * 256, 256, 4004, 2)}
    items = []
    for i in range(TRIP_COUNT):
        p = bytes([i & 0xff]) * (1 + i % 50)
        items.append(big[i] if i in big else (rc._sized([rc.literal(p)]), p))
    return items


def planner_trip_limits(models):
    """[(max_segments, max_units)] (None: room for everything): everything; then one limit ending just in front of item 1030
    (it fits no more) and just behind it (it is the last to fit), units and segments in turn"""
    segs = sum(m.segments for m in models[:1030] if m.split_class)
    units = sum(m.units for m in models[:1030] if m.split_class)
    last = models[1030]
    assert [i for i, m in enumerate(models) if m.split_class] == list(TRIP_SPLIT_AT) and last.units >= 64
    return [(None, None), (None, units), (None, units + last.units), (segs + last.segments - 1, None), (segs + last.segments, None)]


# ---- damaged rich streams, for the independent decoder (raw_cases.expect) ----
MUTATION_SEED, MUTATIONS = 20240618, 600


def damaged_rich_streams():
    """600 seeded mutations of sixteen streams of elements no greedy compressor writes -- twelve fragment-built ones of four
    fragments (flavours 0-3 at fragments of 256, 1,024 and 4,096) and four raw-only ones -- all behind the header, so the
    length stays: a byte changed (four of six), a byte inserted, a truncation.  -> [(stream, the header's length)]"""
    r = np.random.default_rng(MUTATION_SEED)
    sources = [fragment_stream(4 * f, f, 5000 + 4 * k + flavour, flavour)[0] for k, f in enumerate((256, 1024, 4096)) for flavour in range(4)]
    sources += [raw_element_stream((3000, 9000)[k % 2], 5100 + k, k % 3)[0] for k in range(4)]
    out = []
    for k in range(MUTATIONS):
        s = bytearray(sources[int(r.integers(0, len(sources)))])
        n, hdr = rc.header_parses(s)
        at = int(r.integers(hdr, len(s)))
        if k % 6 < 4:
            s[at] ^= int(r.integers(1, 256))
        elif k % 6 == 4:
            s.insert(at, int(r.integers(0, 256)))
        else:
            del s[at:]
        out.append((bytes(s), n))
    return out
