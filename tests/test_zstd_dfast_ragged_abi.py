"""CPU: the ragged zstd level-3 calls of include/lzbench_hip.h 3e without a device -- the sizing functions (the
calls' argument checks: tests/test_ragged_calls_abi.py) and the host mirror of the compact slot placement against the slot
arithmetic recomputed here from the level-3 rows of clevels.h."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import lzbench_amd as L

ZSTD = L.LZH_CODEC_ZSTD
OK, EARG = 0, -1
FAKE = 0x1000   # a non-null "device pointer": the checks under test return before anything reads it
MAX = 16 << 20
SIZES = [0, 1, 6, 7, 63, 64, 65, 255, 1024, 4099, 16384, 16385, 65536, 131072, 131073, 200000, 262144, 262145, 300000,
         1 << 20, (1 << 20) + 1, MAX]
COUNTS = (0, 1, 2, 255, 256, 257, 1000, 16384)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# clevels.h level 3, {windowLog, chainLog, hashLog, minMatch}: sizes above 256 KiB, up to 256 KiB, 128 KiB, 16 KiB
ROWS = ((21, 16, 17, 5), (18, 16, 16, 4), (17, 15, 16, 5), (14, 14, 15, 4))


def align(v):
    return (v + 255) // 256 * 256


def params(n):
    """(hashLog, chainLog, block size) of a frame of n >= 1 bytes: ZSTD_getParams(3, n, 0), adjusted"""
    w, c, h, _ = ROWS[(n <= 262144) + (n <= 131072) + (n <= 16384)]
    src_log = 6 if n < 64 else (n - 1).bit_length()
    w = min(w, src_log)
    h, c = min(h, w + 1), min(c, w)
    return h, c, min(1 << max(w, 10), 131072, n)


def areas(b):
    """the scratch areas before the tables for a block size b: header, sequences, literals, attempt, Huffman stream"""
    return 1024 + align((b // 4 + 16) * 8) + align(b + 64) + align(4 * b + 4096) + align(b + 256)


def stage_slot(n):
    return align(n + (n >> 8) + (((128 << 10) - n) >> 11 if n < (128 << 10) else 0) + 16)


def scratch_slot(n):
    h, c, b = params(max(n, 1))                 # (an empty chunk takes the slot of one byte)
    return align(areas(b) + (4 << h) + (4 << c))


def scratch_worst(maxb):
    """the uniform-slot scratch stride: the areas of maxb's block size, the largest of each table up to maxb"""
    geo = max(maxb, 1)
    cand = [geo, 1] + [1 << lg for lg in range(6, 25) if (1 << lg) < geo]
    hmax, cmax = max(params(n)[0] for n in cand), max(params(n)[1] for n in cand)
    return align(areas(params(geo)[2]) + (4 << hmax) + (4 << cmax))


def arrays_bytes(k):
    """the four per-chunk arrays of the compact layout: two u32 of k, two u64 of k + 1, each 256-aligned"""
    return 2 * align(4 * k) + 2 * align(8 * (k + 1))


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def uni_size(lib, maxb, k, level=3):
    return lib.lzh_zstd_dfast_ragged_compress_temp_bytes(level, maxb, k)


def cmp_size(lib, total, maxb, k, level=3):
    return lib.lzh_zstd_dfast_ragged_compact_compress_temp_bytes(level, total, maxb, k)


@pytest.mark.parametrize("level,maxb", [(1, 65536), (2, 65536), (4, 65536), (-1, 65536), (0, 4096), (19, 4096),
                                        (3, MAX + 1), (1, MAX + 1)])
def test_sizing_is_zero_exactly_where_the_call_refuses(lib, level, maxb):
    out = (C.c_uint64 * 4)()
    one = (C.c_uint64 * 1)(5)
    flag = (C.c_uint8 * 1)()
    assert uni_size(lib, maxb, 4, level) == 0 and cmp_size(lib, 4 * 4096, maxb, 4, level) == 0
    assert lib.lzh_debug_zstd_dfast_ragged_compact_regions(level, 4 * 4096, maxb, 4, out) == EARG
    assert lib.lzh_debug_zstd_dfast_ragged_compact_slots(level, one, 1, maxb, 5, out, out, flag) == EARG


def test_sizing_is_nonzero_for_level_3(lib):
    for maxb in SIZES:
        for k in COUNTS:
            u = uni_size(lib, maxb, k)
            assert (u > 0) == (k > 0), (maxb, k)       # (exactly k slots: nothing for no chunk)
            assert cmp_size(lib, k * maxb, maxb, k) > 0, (maxb, k)


def test_uniform_slot_answer_is_the_formula(lib):
    for maxb in SIZES:
        geo = max(maxb, 1)                              # (a batch of empty chunks: the slots of 1-byte chunks)
        stride = lib.lzh_stage_stride(ZSTD, geo)
        assert stride == stage_slot(geo)
        # the level-3 scratch stride, as the uniform call's sizing has it (two frames' difference)
        uniform_stride = (lib.lzh_compress_temp_bytes(L.LZH_CODEC_ZSTD_DFAST, 2 * geo, geo)
                          - lib.lzh_compress_temp_bytes(L.LZH_CODEC_ZSTD_DFAST, geo, geo) - stride)
        assert uniform_stride == scratch_worst(maxb), maxb
        for k in COUNTS:
            assert uni_size(lib, maxb, k) == k * (stride + uniform_stride), (maxb, k)
    # the worst slot bounds every slot of a size up to it
    for maxb in (63, 64, 16384, 16385, 100000, 131072, 131073, 262144, 262145, 300000):
        ns = set(range(0, min(maxb, 130) + 1)) | {n for s in SIZES for n in (s - 1, s, s + 1) if 0 <= n <= maxb}
        assert max(scratch_slot(n) for n in ns) <= scratch_worst(maxb), maxb
    assert scratch_worst(131072) == scratch_slot(131072) == 1447680


def test_sizing_functions_are_monotone(lib):
    totals = (0, 1, 4096, 100000, 1 << 20, 1 << 24, 1 << 28, 1 << 32, 1 << 36)
    for maxb in SIZES:
        assert [uni_size(lib, maxb, k) for k in COUNTS] == sorted(uni_size(lib, maxb, k) for k in COUNTS)
    for k in COUNTS:
        assert [uni_size(lib, m, k) for m in SIZES] == sorted(uni_size(lib, m, k) for m in SIZES)
    for maxb in SIZES:
        for k in COUNTS:
            v = [cmp_size(lib, t, maxb, k) for t in totals]
            assert v == sorted(v), (maxb, k)
    for t in totals:
        for maxb in SIZES:
            v = [cmp_size(lib, t, maxb, k) for k in COUNTS]
            assert v == sorted(v), (t, maxb)
        for k in COUNTS:
            v = [cmp_size(lib, t, m, k) for m in SIZES]
            assert v == sorted(v), (t, k)


def test_compact_answer_is_within_the_uniform_slot_answer(lib):
    for maxb in SIZES:
        for k in COUNTS:
            for t in (0, 1, 4096 * k, k * maxb // 2, k * maxb, 1 << 40):
                assert cmp_size(lib, t, maxb, k) <= uni_size(lib, maxb, k) + arrays_bytes(k), (t, maxb, k)
    # the skewed batch of the GPU test: below a tenth of the uniform-slot temp
    assert 10 * cmp_size(lib, 255 * 4096 + (1 << 20), 1 << 20, 256) < uni_size(lib, 1 << 20, 256)


def mirror(lib, sizes, maxb, total):
    k = len(sizes)
    a = (C.c_uint64 * k)(*sizes)
    so, ro, pr = (C.c_uint64 * k)(), (C.c_uint64 * k)(), (C.c_uint8 * k)()
    assert lib.lzh_debug_zstd_dfast_ragged_compact_slots(3, a, k, maxb, total, so, ro, pr) == OK
    reg = (C.c_uint64 * 4)()
    assert lib.lzh_debug_zstd_dfast_ragged_compact_regions(3, total, maxb, k, reg) == OK
    return list(so), list(ro), list(pr), list(reg)


POOL = [0, 1, 63, 64, 65, 16384, 16385, 131072, 131073, 262144, 262145]


def size_list(seed):
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, 48))
    top = int(rng.choice([70, 5000, 20000, 140000, 300000]))
    sizes = [int(rng.choice(POOL)) if rng.random() < 0.5 else int(rng.integers(0, top + 1)) for _ in range(k)]
    if seed % 5 == 0:
        sizes[int(rng.integers(0, k))] = MAX
    return sizes


def test_placement_of_promise_keeping_batches(lib):
    seen = set()
    for seed in range(200):
        sizes = size_list(seed)
        maxb, total, k = max(sizes) + (seed % 3) * 1000 * (max(sizes) < MAX), sum(sizes), len(sizes)
        so, ro, pr, reg = mirror(lib, sizes, maxb, total)
        assert all(pr), (seed, sizes)
        assert reg[0] % 256 == 0 and reg[2] % 256 == 0
        assert reg[0] + reg[1] <= reg[2] and reg[2] + reg[3] <= cmp_size(lib, total, maxb, k)
        s_at = r_at = 0
        for i, n in enumerate(sizes):
            # exclusive scans of the slot sizes recomputed here: the slots are those sizes and do not overlap
            assert so[i] == s_at and ro[i] == r_at, (seed, i, n)
            assert so[i] % 256 == 0 and ro[i] % 256 == 0
            s_at += stage_slot(n)
            r_at += scratch_slot(n)
            assert s_at <= reg[1] and r_at <= reg[3], (seed, i, n)
        seen.update(sizes)
    assert set(POOL) <= seen and MAX in seen


def test_a_batch_that_breaks_the_promise(lib):
    dropped = 0
    for seed in range(40):
        sizes = size_list(1000 + seed) + [5000] * 8
        maxb = max(sizes)
        if seed % 2:                                                    # (odd seeds: one chunk over max_bytes too)
            sizes[1] = maxb + 1
        total = sum(s for s in sizes if s <= maxb) // 3
        so, ro, pr, reg = mirror(lib, sizes, maxb, total)
        s_at = r_at = 0
        for i, n in enumerate(sizes):
            over = n > maxb
            ss, rs = (0, 0) if over else (stage_slot(n), scratch_slot(n))
            assert so[i] == s_at and ro[i] == r_at
            inside = s_at + ss <= reg[1] and r_at + rs <= reg[3]
            assert pr[i] == (1 if inside and not over else 0), (seed, i, n)
            s_at += ss
            r_at += rs
        dropped += len(sizes) - sum(pr)
    assert dropped > 40                                                 # the promise was indeed broken


def test_recorded_answers(lib):
    """the two standard batches of include/lzbench_hip.h 3e"""
    with open(os.path.join(GOLD, "sizing_zstd_dfast_ragged.json")) as f:
        rec = json.load(f)["batches"]
    assert [b["name"] for b in rec] == ["one-16MiB-and-4095-of-4KiB", "4096-of-128KiB"]
    assert (rec[0]["total_in_bytes"], rec[1]["total_in_bytes"]) == (MAX + 4095 * 4096, 4096 * 131072)
    for b in rec:
        assert b["nchunks"] == 4096
        assert cmp_size(lib, b["total_in_bytes"], b["max_chunk_bytes"], b["nchunks"]) == b["compact_temp_bytes"]
        assert uni_size(lib, b["max_chunk_bytes"], b["nchunks"]) == b["uniform_slot_temp_bytes"]
    assert 60 * rec[0]["compact_temp_bytes"] < rec[0]["uniform_slot_temp_bytes"]
    assert rec[1]["compact_temp_bytes"] - rec[1]["uniform_slot_temp_bytes"] == arrays_bytes(4096)


def test_the_calls_of_3b_and_3c_still_refuse_level_3(lib):
    DF = L.LZH_CODEC_ZSTD_DFAST
    assert lib.lzh_ragged_compress_temp_bytes(DF, 65536, 4) == 0
    assert lib.lzh_compress_ragged_async(DF, 3, FAKE, FAKE, 4, 65536, FAKE, 1 << 20, FAKE, FAKE, FAKE, 1 << 40, None) == EARG
    assert lib.lzh_zstd_ragged_compress_temp_bytes(3, 65536, 4) == 0
    assert lib.lzh_zstd_ragged_compact_compress_temp_bytes(3, 4 * 65536, 65536, 4) == 0
    assert lib.lzh_zstd_compress_ragged_async(3, FAKE, FAKE, 4, 65536, FAKE, 1 << 20, FAKE, FAKE, FAKE, 1 << 40, None) == EARG


def test_python_class_refusals():
    """RaggedCodec's checks come before any torch call: no device needed."""
    for kw in (dict(level=1), dict(level=2), dict(level=0), dict(level=3, compact=True),
               dict(level=3, dictionary=np.zeros(64, np.uint8))):
        with pytest.raises(ValueError):
            L.RaggedCodec("zstd_dfast", 65536, 4, **kw)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd_dfast", MAX + 1, 4, level=3)
