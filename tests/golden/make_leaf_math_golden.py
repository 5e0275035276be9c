"""Writes tests/golden/leaf_math_sha256.json: one sha256 per math sweep of tests/test_device_leaves.py, with the
point counts, from THIS host's libm -- powf, logf, log10f and the two double expressions of the old VBR loop
(reference quantize.c:1419-1426), evaluated by tests/gpu_tools/lh_leaf_libm.c over exactly the sweeps of
tests/leaf_support.py.  The authority is the libm the reference was built with, glibc 2.35: run it there, after
`make -C tests/gpu_tools', as

    python tests/golden/make_leaf_math_golden.py
"""
import json
import os
import platform
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import leaf_support  # noqa: E402


def main():
    out = {}
    for name, (op, a, b, flag) in leaf_support.libm_sweeps().items():
        out[name] = {"points": int(a.size), "sha256": leaf_support.sha(leaf_support.libm(op, a, b, flag))}
        print("%-28s %9d points  %s" % (name, a.size, out[name]["sha256"]))
    out["_libm"] = " ".join(platform.libc_ver())
    with open(leaf_support.DIGESTS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
