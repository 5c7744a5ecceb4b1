"""The zstd level-3 fixture (tests/golden/zstd_dfast_golden.json) on the CPU: the committed digests are what the
reference build writes today for the inputs of tests/zstd_dfast_cases.py, and every reference frame decodes back to
its input.  Both need the reference build (oracle/_ref) and skip without it; the C restatement under oracle/ covers
zstd's fast-strategy compressor only and has no zstd decoder, so the frames are decoded by the reference build's."""
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import zstd_dfast_cases as Z

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)


def golden():
    with open(os.path.join(GOLD, "zstd_dfast_golden.json")) as f:
        return json.load(f)


def test_fixture_lists_every_case_once():
    g = golden()["cases"]
    assert [(c["name"], c["corpus"], c["n"], c["chunk"]) for c in g] == Z.cases()
    assert len({c["name"] for c in g}) == len(g)
    assert all(c["level"] == 3 and c["seed"] == Z.SEED for c in g)


@pytest.mark.parametrize("case", golden()["cases"], ids=lambda c: c["name"])
def test_reference_build_reproduces_digests_and_frames_decode(case):
    if not O.have_ref():
        pytest.skip("reference build (oracle/_ref) not present")
    import make_zstd_dfast_golden as M
    assert golden()["version"] == int(O.ref().ref_zstd_version())
    assert M.entry(case["name"], case["corpus"], case["n"], case["chunk"]) == case
    data = Z.corpus(case["corpus"], case["n"])
    packed, cs = M.reference(data, case["chunk"])
    off = 0
    for i, part in enumerate(int(v) for v in Z.chunk_list(case["n"], case["chunk"])):
        clen = int(cs[i])
        src = data[i * case["chunk"]:i * case["chunk"] + part]
        if clen == part:                       # the raw-store rule
            assert packed[off:off + clen].tobytes() == src.tobytes()
        else:
            frame = np.ascontiguousarray(packed[off:off + clen])
            out = np.zeros(part + 64, np.uint8)
            assert O.ref().ref_zstd_decompress(frame.ctypes.data, clen, out.ctypes.data, part) == part
            assert out[:part].tobytes() == src.tobytes()
        off += clen
    assert off == len(packed)
