#!/usr/bin/env python3
"""Are the kernels of one build of the device code the same as another's?  Compares, kernel by kernel, the text between a
kernel's label and its .end_amdhsa_kernel in two assembly files made with
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S pim-compression_amd/csrc/snappy_hip.hip -o FILE
Local labels carry the number of the function in the file (.LBB13_4), which shifts for every kernel emitted behind a new one
(template instantiations come last); that number is masked, nothing else.  Prints SAME / DIFF per kernel of the first file,
NEW for kernels only the second has; exit status 1 if any kernel differs or is gone.
Usage: python tools/kernel_asm_diff.py before.s after.s
"""
import re
import sys


def kernels(path):
    with open(path) as f:
        text = f.read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
        m = re.search(r"^(" + re.escape(name) + r"):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
        out[name] = re.sub(r"BB\d+_", "BBn_", re.sub(r"\.L(func_end|tmp)\d+", ".Lx", m.group(2)))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in a:
        same = a[name] == b.get(name)
        bad += not same
        print(("SAME " if same else "DIFF ") + name)
    for name in b:
        if name not in a:
            print("NEW  " + name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
