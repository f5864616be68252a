"""Cases of the split check of raw Snappy streams (snappy_hip_raw_check_split_batch), shared by the emulator
and the GPU tests, and a MODEL of its result words in plain Python that shares no code with the kernels.

The call's verdicts are the serial checker's whatever steps 2-4 do, so a mistake there shows in the four result words alone: a
valid large stream that is not proven by the parallel path merely costs the serial time.  words() says what they must be for
ANY stream: an item settled by its header is in none of them; one with at most one segment is SMALL; every other one is SPLIT
iff the independent decoder (raw_cases.expect, with a sufficient capacity) accepts it and FELL_BACK if not.  The nodes step 3
leaves are those of raw_split_cases.model, which does not depend on the unit.  The hand-made streams put a copy of every kind
into the first, a middle and the last node of a stream, in the node's first window and deeper, with an offset that reaches the
stream's very first output byte, one a byte larger and one of 0; where each copy sits is computed from the model, so the inputs
cannot quietly stop covering a case."""
import datagen
import raw_cases as rc
import raw_split_cases as sc

SPLIT, SMALL, FELL_BACK, SETTLED = [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]
DEFAULT_SEGMENT = 16384
ANY_UNIT = 256


# ---- the model ----
def segments(stream, segment_bytes):
    """segments of a stream whose header parses"""
    return -(-(len(stream) - rc.header_parses(stream)[1]) // segment_bytes)


def is_large(stream, segment_bytes, null_src=False):
    h = None if null_src else rc.header_parses(stream)
    return bool(h) and 0 < h[0] <= rc.RAW_MAX_LEN and len(stream) <= rc.RAW_MAX_LEN and segments(stream, segment_bytes) > 1


def words(stream, segment_bytes, null_src=False):
    """the result words of one item that is inside max_segments"""
    h = None if null_src else rc.header_parses(stream)
    if h is None or h[0] == 0 or h[0] > rc.RAW_MAX_LEN or len(stream) > rc.RAW_MAX_LEN:
        return SETTLED
    if segments(stream, segment_bytes) <= 1:
        return SMALL
    return SPLIT if rc.expect(stream, rc.RAW_MAX_LEN)[0] == rc.OK else FELL_BACK


def batch_words(streams, segment_bytes, max_segments=None):
    """the four result words of one call: the sum of the items' words, with every large item from the first one that does not
    fit max_segments on handed to the serial checker, as the plan does it (raw_split_cases.batch_words, without units)"""
    total, segs = [0, 0, 0, 0], 0
    for s in streams:
        w = words(s, segment_bytes)
        if is_large(s, segment_bytes):
            segs += segments(s, segment_bytes)
            if max_segments is not None and segs > max_segments:
                w = FELL_BACK
        total = [a + b for a, b in zip(total, w)]
    return total


def expected(stream, null_src=False):
    """(status, out_len) of one item: raw_cases.expect with a sufficient capacity"""
    if null_src:
        return rc.INVALID, 0
    st, n, _ = rc.expect(stream, rc.RAW_MAX_LEN)
    return st, n


def nodes(stream, segment_bytes):
    """what step 3 must leave for a VALID large stream: one (entry, landing, output base) or None per segment"""
    m = sc.model(stream, ANY_UNIT, segment_bytes)
    return [m.nodes.get(s) for s in range(m.segments)]


# ---- hand-made streams: copies at their absolute output position (segments of 128 bytes, headers of 2 bytes) ----
HAND_SEGMENT = 128
COPIES = (("copy_1", rc.copy1), ("copy_2", rc.copy2), ("copy_4", rc.copy4))
WHERE, DEPTH = ("first", "middle", "last"), ("window_0", "deeper")


def _hand_stream(copy, literal_bytes, after, offset, seed):
    """`after` literals, a 4-byte copy at `offset`, more literals up to 26 elements, 9 bytes at the end"""
    data = datagen.random_bytes(26 * literal_bytes + 9, seed=seed)
    lits = [rc.literal(data[k * literal_bytes:(k + 1) * literal_bytes]) for k in range(25)] + [rc.literal(data[-9:])]
    return rc._sized(lits[:after] + [copy(4, offset)] + lits[after:])


def _place(stream, copy_at):
    """(where, depth) of the element at compressed position copy_at, from the model's nodes alone"""
    ns = [n for n in nodes(stream, HAND_SEGMENT) if n is not None]
    k = next(k for k, (entry, landing, _) in enumerate(ns) if entry <= copy_at < landing)
    where = "first" if k == 0 else "last" if k == len(ns) - 1 else "middle"
    return where, "window_0" if (copy_at - ns[k][0]) // 64 == 0 else "deeper"


def hand_streams():
    """name -> (stream, (status, result words)): for every kind of copy, every place (first / middle / last node) and every
    depth (the node's first 64-byte window / a later one) a copy whose offset is exactly its absolute output position (it reads
    the stream's first output byte: valid, SPLIT), one a byte larger and one of 0 (both INVALID, FELL_BACK)"""
    v, found = {}, set()
    for k, (kind, copy) in enumerate(COPIES):
        for literal_bytes in (59, 47, 38):
            for after in range(1, 26):
                position = after * literal_bytes                      # the copy's absolute output position
                if position + 1 >= (2048 if kind == "copy_1" else 65536):
                    continue
                s = _hand_stream(copy, literal_bytes, after, position, 700 + k)
                hdr = rc.header_parses(s)[1]
                where, depth = _place(s, hdr + after * (literal_bytes + 1))
                if (kind, where, depth) in found:
                    continue
                found.add((kind, where, depth))
                name = "%s_%s_%s" % (kind, where, depth)
                v[name + "_reaches_first_byte"] = (s, (rc.OK, SPLIT))
                v[name + "_one_beyond"] = (_hand_stream(copy, literal_bytes, after, position + 1, 700 + k), (rc.INVALID, FELL_BACK))
                v[name + "_offset_0"] = (_hand_stream(copy, literal_bytes, after, 0, 700 + k), (rc.INVALID, FELL_BACK))
    assert found == {(kind, w, d) for kind, _ in COPIES for w in WHERE for d in DEPTH}, \
        sorted({(kind, w, d) for kind, _ in COPIES for w in WHERE for d in DEPTH} - found)
    for name, (s, (st, w)) in v.items():
        assert rc.header_parses(s)[1] == 2 and expected(s)[0] == st and words(s, HAND_SEGMENT) == w, name
    return v


# ---- more items than one trip of the planner ----
def planner_trip_limits(streams, segment_bytes):
    """[max_segments] (None: room for everything): everything; the limit ending just in front of the last large item, one
    segment short of it, and exactly behind it"""
    large = [i for i, s in enumerate(streams) if is_large(s, segment_bytes)]
    assert large == list(sc.TRIP_SPLIT_AT), large
    before = sum(segments(streams[i], segment_bytes) for i in large[:-1])
    last = segments(streams[large[-1]], segment_bytes)
    return [None, before, before + last - 1, before + last]
