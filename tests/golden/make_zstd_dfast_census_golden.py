#!/usr/bin/env python3
"""tests/golden/make_zstd_dfast_census_golden.py -- golden digests for zstd level-3 compression of the named inputs
of tests/zstd_dfast_inputs.py, each as one chunk of its own size: the reference zstd 1.5.2 build through lzbench's
chunk loop, exactly as tests/golden/make_zstd_dfast_golden.py (whose reference() this uses).  Stored per input: n, the
packed byte count, sha256 of the compr_sizes, of the packed stream and of the input; the inputs regenerate from their
seeds.  Data only.
Run from the repo root:  python tests/golden/make_zstd_dfast_census_golden.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import oracle_lib as O  # noqa: E402
import zstd_dfast_inputs as I  # noqa: E402
from make_zstd_dfast_golden import reference  # noqa: E402


def entry(inp):
    data = inp.make()
    packed, cs = reference(data, len(data))
    assert len(cs) == 1
    return dict(name=inp.name, n=int(len(data)), level=3,
                input_sha256=hashlib.sha256(data.tobytes()).hexdigest(),
                packed_sha256=hashlib.sha256(packed.tobytes()).hexdigest(),
                csizes_sha256=hashlib.sha256(cs.astype("<u8").tobytes()).hexdigest(),
                packed_bytes=int(len(packed)))


def main():
    cases = [entry(i) for i in I.INPUTS]
    for c in cases:
        print(c["name"], c["n"], c["packed_bytes"], flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "zstd_dfast_census_golden.json"), "w") as f:
        json.dump({"generator": "zstd 1.5.2 reference build (oracle/_ref), tests/golden/make_zstd_dfast_census_golden.py",
                   "version": int(O.ref().ref_zstd_version()), "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
