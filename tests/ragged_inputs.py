"""The cases, the edge-size batch and the expected bytes that the GPU tests of the LZ4 and snappy ragged calls share
(test_gpu_ragged.py, test_gpu_ragged_compact.py, test_gpu_temp_guards.py, test_gpu_lzc_census.py).  No tests."""
import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
from gpu_batches import layout

# (codec name, level): LZ4_compress_default, LZ4_compress_fast at acceleration 7, snappy
CASES = [("lz4", 1), ("lz4fast", 7), ("snappy", 0)]
CASE_IDS = ["lz4", "lz4-acc7", "snappy"]
# 65546 | 65547: LZ4's byU16 / byU32 tables; 14 | 15: snappy's all-literal bound; 200000: four snappy fragments
EDGE_SIZES = [70000, 0, 1, 12, 13, 14, 15, 16, 255, 4099, 65535, 65536, 65546, 65547, 200000, 3]

_expect_cache = {}


def expect(chunk: np.ndarray, codec: str, level: int) -> bytes:
    """The packed bytes of one chunk from the CPU oracle (raw-store rule applied; cached), checked against the
    reference build's own functions where that is present."""
    key = (chunk.tobytes(), codec, level)
    if key not in _expect_cache:
        if len(chunk):
            packed, cs = O.compress_chunks(np.ascontiguousarray(chunk), codec, len(chunk), level)
            assert len(cs) == 1 and int(cs[0]) == len(packed)
        else:   # (the oracle's chunk loop has no chunk for an empty input: its block functions, one byte each)
            empty = np.zeros(1, np.uint8)[:0]
            packed = np.frombuffer(O.snappy_compress(empty) if codec == "snappy" else O.lz4_compress(empty, max(level, 1)),
                                   np.uint8)
            assert len(packed) == 1
        if O.have_ref():
            R = O.ref()
            src = np.ascontiguousarray(chunk) if len(chunk) else np.zeros(1, np.uint8)
            dst = np.zeros(len(chunk) + len(chunk) // 6 + 1024, np.uint8)
            if codec == "snappy":
                r = R.ref_snappy_compress(src.ctypes.data, len(chunk), dst.ctypes.data)
            else:   # (ref_lz4_compress_fast at acceleration 1 is LZ4_compress_default)
                r = R.ref_lz4_compress_fast(src.ctypes.data, dst.ctypes.data, len(chunk), len(dst), max(level, 1))
            ref = chunk.tobytes() if r == len(chunk) else dst[:r].tobytes()
            assert ref == packed.tobytes(), "oracle and reference build differ"
        _expect_cache[key] = packed.tobytes()
    return _expect_cache[key]


def expected(host, offs, sizes, codec, level):
    """check_batch's `expected` for chunks laid out in host: chunk index -> expect() of that chunk's bytes"""
    return lambda i: expect(host[offs[i]: offs[i] + sizes[i]], codec, level)


@pytest.fixture(scope="module")
def edge_input():
    offs, total = layout(EDGE_SIZES)
    return L.datagen("text", total, seed=21), offs


def raw_chunk(codec):
    """4096 bytes whose compressed size is 4096 (found by a CPU search over the oracle: random bytes of seed 1
    with one short run; LZ4: the last 37 bytes, snappy: bytes 100..114)."""
    d = L.datagen("random", 4096, seed=1).copy()
    if codec == "snappy":
        d[100:115] = 0x42
    else:
        d[4096 - 37:] = 0x41
    return d
