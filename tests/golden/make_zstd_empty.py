"""tests/golden/make_zstd_empty.py -- the frame the REFERENCE build (oracle/_ref/libref.so, zstd 1.5.2) writes
for an empty input at the levels the GPU codec compresses, with lzbench's zstd row semantics
(ZSTD_getParams(level, 0, 0), contentSizeFlag = 1, ZSTD_compress_advanced).  The CPU restatement's chunk loop
has no chunk for an empty input, so the zero-length chunk of a ragged batch is checked against this fixture.
Run from the repo root:
    python tests/golden/make_zstd_empty.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402

LEVELS = [1, 2, -1, -2, -3, -4, -5]


def main():
    R = O.ref()
    frames = {}
    for level in LEVELS:
        src, dst = np.zeros(1, np.uint8), np.zeros(64, np.uint8)
        r = R.ref_zstd_compress(src.ctypes.data, 0, dst.ctypes.data, len(dst), level)
        assert r > 0
        frames[str(level)] = dst[:r].tobytes().hex()
    with open(os.path.join(ROOT, "tests", "golden", "zstd_empty.json"), "w") as f:
        json.dump({"generator": "zstd 1.5.2 reference build (oracle/_ref)", "version": int(R.ref_zstd_version()),
                   "frames": frames}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
