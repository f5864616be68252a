"""Times the four single-device drop-in calls of one build: python tools/phased_calls.py TREE OUT.json  (TREE = a built checkout, e.g. "." or a copy of another commit)
20 warm repetitions each (the first call of the process, which creates streams and starts the copy engines, is discarded):
wall seconds around the binding's call and the sum of the call's program_runtime fields."""
import hashlib
import json
import os
import sys
import time

tree, out = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, os.path.join(tree, "pim-compression_amd"))
import snappy_hip_binding as shb  # noqa: E402

assert shb.LIB_PATH.startswith(tree), shb.LIB_PATH
golden = os.path.join(tree, "tests", "golden")
xml = open(os.path.join(golden, "xml.snappy"), "rb").read()
world = open(os.path.join(golden, "world192.txt"), "rb").read()
off, n = (1 << 20) + 12345, 1 << 20
patch = bytes((i * 131 + (i >> 9)) & 0xff for i in range(n))
st, raw, _ = shb.raw_compress_host(world)
assert st == 0
calls = {
    "range xml.snappy 1 MiB": lambda: shb.decompress_range_host(xml, off, n),
    "update xml.snappy 1 MiB": lambda: shb.update_range_host(xml, off, patch),
    "raw compress world192.txt": lambda: shb.raw_compress_host(world),
    "raw decode world192.txt": lambda: shb.raw_decompress_host(raw),
}
res = {"lib": shb.LIB_PATH}
for name, fn in calls.items():
    fn()
    wall, rt_sum, digest = [], [], None
    for _ in range(20):
        t = time.perf_counter()
        st, got, rt = fn()
        wall.append(time.perf_counter() - t)
        assert st == 0
        rt_sum.append(sum(rt[k] for k in ("pre", "d_alloc", "load", "copy_in", "run", "copy_out", "d_free")))
        d = hashlib.sha256(got).hexdigest()
        assert digest in (None, d)
        digest = d
    res[name] = {"wall_s": wall, "runtime_sum_s": rt_sum, "sha256": digest, "bytes": len(got), "last_runtime": rt}
    print(name, "wall median %.3f ms" % (sorted(wall)[10] * 1e3), "runtime sum median %.3f ms" % (sorted(rt_sum)[10] * 1e3), flush=True)
json.dump(res, open(out, "w"))
