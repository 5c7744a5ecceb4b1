#!/usr/bin/env python3
"""tests/golden/make_lz4hc.py -- LZ4 blocks written by the REFERENCE lz4 1.9.3 HC parser (LZ4_compress_HC through
oracle/_ref/libref.so): valid blocks that the fast parser, the only one this project restates, never writes.  HC
streams are dense in 3-byte sequences (no literals, a short match) and pick far offsets the fast parser's single
hash probe does not find.

Stored: the streams (lz4hc.npz, a file under 64 KiB) and, per case, the corpus and seed that regenerate its
16 KiB input, the input's sha256 and the stream's size and sha256 (lz4hc.json).  The inputs are not stored.
Run from the repo root:  python tests/golden/make_lz4hc.py"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lzbench_amd as L  # noqa: E402
import oracle_lib as O  # noqa: E402

N = 16384
SEED = 31
CASES = [(corpus, level) for corpus in ("text", "binary") for level in (4, 9, 12)]


def compress_hc(data: np.ndarray, level: int) -> bytes:
    assert O.have_ref_hc(), "build oracle/_ref with the HC shim first (make -C oracle ref)"
    out = np.zeros(len(data) + len(data) // 255 + 64, np.uint8)
    r = O.ref().ref_lz4_compress_hc(data.ctypes.data, out.ctypes.data, len(data), len(out), level)
    assert r > 0
    return out[:r].tobytes()


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    arrays, meta = {}, []
    for corpus, level in CASES:
        data = L.datagen(corpus, N, seed=SEED)
        s = compress_hc(data, level)
        name = f"{corpus}_l{level}"
        arrays[name] = np.frombuffer(s, np.uint8)
        meta.append({"name": name, "corpus": corpus, "seed": SEED, "n": N, "level": level,
                     "input_sha256": hashlib.sha256(data.tobytes()).hexdigest(),
                     "stream_bytes": len(s), "stream_sha256": hashlib.sha256(s).hexdigest()})
    np.savez_compressed(os.path.join(here, "lz4hc.npz"), **arrays)
    assert os.path.getsize(os.path.join(here, "lz4hc.npz")) < 65536
    with open(os.path.join(here, "lz4hc.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print({m["name"]: m["stream_bytes"] for m in meta})


if __name__ == "__main__":
    main()
