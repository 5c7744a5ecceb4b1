#!/usr/bin/env python3
"""tests/golden/make_zstd_dfast_golden.py -- golden digests for zstd COMPRESSION at level 3 (the hip_zstd_dfast
row, LZH_CODEC_ZSTD_DFAST): the reference zstd 1.5.2 build (oracle/_ref/libref.so, lzbench's zstd row semantics:
ZSTD_getParams(3, chunk, 0) + contentSizeFlag + ZSTD_compress_advanced) run through lzbench's chunk loop (raw-store
rule, contiguous packing) on the inputs of tests/zstd_dfast_cases.py.  Stored per case: corpus, seed, n, chunk, the
packed byte count, sha256 of the compr_sizes (little-endian u64), of the packed stream and of the input; inputs
regenerate from the seeds.  Data only.
Run from the repo root:  python tests/golden/make_zstd_dfast_golden.py"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import zstd_dfast_cases as Z  # noqa: E402


def reference(data, chunk):
    """(packed, compr_sizes) of the reference build; the empty input is one empty chunk"""
    if len(data) == 0:
        dst = np.zeros(1024, np.uint8)
        r = O.ref().ref_zstd_compress(np.zeros(1, np.uint8).ctypes.data, 0, dst.ctypes.data, len(dst), Z.LEVEL)
        assert r > 0
        return dst[:r].copy(), np.array([r], np.uint64)
    return O.compress_chunks(data, "zstd", chunk, Z.LEVEL, use_ref=True)


def entry(name, kind, n, chunk):
    data = Z.corpus(kind, n)
    assert len(data) == n, (name, len(data))
    packed, cs = reference(data, chunk)
    return dict(name=name, corpus=kind, seed=Z.SEED, n=n, chunk=chunk, level=Z.LEVEL,
                input_sha256=hashlib.sha256(data.tobytes()).hexdigest(),
                packed_sha256=hashlib.sha256(packed.tobytes()).hexdigest(),
                csizes_sha256=hashlib.sha256(cs.astype("<u8").tobytes()).hexdigest(),
                packed_bytes=int(len(packed)))


def main():
    cases = []
    for c in Z.cases():
        cases.append(entry(*c))
        print(cases[-1]["name"], cases[-1]["n"], cases[-1]["chunk"], cases[-1]["packed_bytes"], flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "zstd_dfast_golden.json"), "w") as f:
        json.dump({"generator": "zstd 1.5.2 reference build (oracle/_ref), tests/golden/make_zstd_dfast_golden.py",
                   "version": int(O.ref().ref_zstd_version()), "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
