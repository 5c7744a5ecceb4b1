"""The edge-size batch, the corpus and the expected frames that the GPU tests of the ragged zstd calls share
(test_gpu_zstd_ragged*.py, test_gpu_zstd_census.py, test_gpu_zstd_dfast_ragged.py).  No tests."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
from gpu_batches import layout

# 6 | 7: ZSTD_buildSeqStore's raw-block bound; 16384 | 16385, 131072 | 131073, 262144 | 262145: the ZSTD_getParams
# size classes; 131073 and 262145: the two- and three-block boundaries
EDGE_SIZES = [0, 1, 6, 7, 8, 255, 4099, 16383, 16384, 16385, 65536, 131071, 131072, 131073, 262144, 262145, 300000]
EDGE_L2 = [s for s in EDGE_SIZES if s <= 131072]      # level 2 is the fast strategy up to 128 KiB chunks only
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def codec_name(level):
    return "zstd" if level > 0 else "zstd_fast"


def corpus_mix(n, seed):
    """n bytes: datagen("mixed") then datagen("text"), half each"""
    h = n // 2
    return np.concatenate([L.datagen("mixed", h, seed=seed), L.datagen("text", n - h, seed=seed + 1)])


_empty = None
_expect_cache = {}


def expect(chunk: np.ndarray, level: int) -> bytes:
    """The packed bytes of one chunk: the frame of the CPU restatement for a chunk of that size alone (raw-store
    rule applied; cached), checked against the reference build's ZSTD_compress_advanced where that is present.
    An empty chunk: the reference's frame for 0 bytes (tests/golden/zstd_empty.json)."""
    global _empty
    key = (chunk.tobytes(), level)
    if key not in _expect_cache:
        if len(chunk) == 0:
            if _empty is None:
                with open(os.path.join(GOLD, "zstd_empty.json")) as f:
                    _empty = json.load(f)["frames"]
            packed = bytes.fromhex(_empty[str(level)])
        else:
            p, cs = O.compress_chunks(np.ascontiguousarray(chunk), "zstd", len(chunk), level, use_ref=False)
            assert len(cs) == 1 and int(cs[0]) == len(p)
            packed = p.tobytes()
        if O.have_ref():
            src = np.ascontiguousarray(chunk) if len(chunk) else np.zeros(1, np.uint8)
            dst = np.zeros(len(chunk) + len(chunk) // 128 + 1024, np.uint8)
            r = O.ref().ref_zstd_compress(src.ctypes.data, len(chunk), dst.ctypes.data, len(dst), level)
            ref = chunk.tobytes() if r <= 0 or r == len(chunk) else dst[:r].tobytes()
            assert ref == packed, f"restatement and reference build differ ({len(chunk)} bytes, level {level})"
        _expect_cache[key] = packed
    return _expect_cache[key]


def expected(host, offs, sizes, level):
    """check_batch's `expected` for chunks laid out in host: chunk index -> expect() of that chunk's bytes"""
    return lambda i: expect(host[offs[i]: offs[i] + sizes[i]], level)


@pytest.fixture(scope="module")
def edge_input():
    offs, total = layout(EDGE_SIZES)
    return corpus_mix(total, 21), offs
