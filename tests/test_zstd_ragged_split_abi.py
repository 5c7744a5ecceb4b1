"""CPU: the split-decoder side of the ragged zstd calls (include/lzbench_hip.h 3c) without a device -- the
sizing function and the debug layout it shares with the launcher (the async call's argument checks, the same whatever
temp_bytes is: tests/test_ragged_calls_abi.py)."""
import numpy as np
import pytest

import lzbench_amd as L

ZSTD = L.LZH_CODEC_ZSTD
OK, EARG = 0, -1
MAX = 16 << 20
SPLIT_MIN = 16384
SIZES = [SPLIT_MIN, 16385, 65536, 70000, 131072, 131073, 200000, 262144, 262145, 300000, 1 << 20, (1 << 20) + 1, MAX]
COUNTS = [0, 1, 2, 7, 8, 9, 255, 256, 257, 1000, 8192, 16384]
REGIONS = ["offsets", "frames", "dummy", "states", "fields", "njobs", "jobs"]


def split_bytes(maxb, k):
    return L.lib().lzh_zstd_ragged_decompress_split_temp_bytes(maxb, k)


def small_bytes(maxb, k):
    return L.lib().lzh_zstd_ragged_decompress_temp_bytes(maxb, k)


def temp_layout(maxb, k):
    out = np.zeros(16, np.uint64)
    rc = L.lib().lzh_debug_zstd_ragged_split_layout(maxb, k, out.ctypes.data)
    return rc, [int(v) for v in out]


def test_the_symbols_exist():
    lib = L.lib()
    assert lib.lzh_zstd_ragged_decompress_split_temp_bytes is not None
    assert lib.lzh_debug_zstd_ragged_split_layout is not None


def test_where_there_is_a_split_decoder():
    for k in (0, 1, 4, 1000):
        assert split_bytes(SPLIT_MIN - 1, k) == 0
        assert split_bytes(MAX + 1, k) == 0
        assert split_bytes(0, k) == 0
        assert split_bytes(SPLIT_MIN, k) > 0
        assert split_bytes(MAX, k) > 0


def test_sizing_is_monotone_and_never_below_the_one_wave_answer():
    for maxb in SIZES:
        prev = 0
        for k in COUNTS:
            v = split_bytes(maxb, k)
            assert v >= prev and v > 0, (maxb, k)
            assert v >= small_bytes(maxb, k) > 0, (maxb, k)
            prev = v
    for k in COUNTS:
        prev = 0
        for maxb in SIZES:
            v = split_bytes(maxb, k)
            assert v >= prev, (maxb, k)
            prev = v


def test_sizing_follows_the_uniform_decoders_layout():
    """Both answers come from the same per-frame layout (the uniform one also holds the plan's frame list)."""
    lib = L.lib()
    for maxb in [s for s in SIZES if s <= (1 << 20) + 1]:
        for k in [c for c in COUNTS if c > 0]:
            uni = lib.lzh_decompress_temp_bytes(ZSTD, k * maxb, maxb)
            assert abs(split_bytes(maxb, k) - uni) <= 64 * k + 4096, (maxb, k, split_bytes(maxb, k), uni)
    assert abs(split_bytes(MAX, 3) - lib.lzh_decompress_temp_bytes(ZSTD, 3 * MAX, MAX)) <= 64 * 3 + 4096


def test_uniform_and_ragged_sizes_differ_by_a_closed_form():
    """The uniform and the ragged call describe the same per-frame layout: frames, dummy words, states, fields and
    the job counter are the same bytes in both, so the two published answers differ by exactly the plan list, the
    rounding of the jobs region and the two scan regions' gaps:
      uniform = align(8 (k + 1))       + shared + (jobs + 256)        + align(4 k + 8) + 256
      ragged  = align(8 (k + 1)) + 256 + shared + (align(jobs) + 256)
    with align to 256 and jobs = k frames x (blocks of 128 KiB in maxb, and one) x 64 bytes a Huffman job."""
    lib = L.lib()

    def align(v):
        return (v + 255) // 256 * 256

    for maxb in SIZES:
        for k in [c for c in COUNTS if c > 0]:
            jobs = k * ((maxb + 131071) // 131072 + 1) * 64
            assert temp_layout(maxb, k)[1][13] == jobs, (maxb, k)
            plan = align(4 * k + 8)             # the uniform call's frame list and two counts
            rounding = align(jobs) - jobs       # the ragged call rounds its jobs region, the uniform one does not
            gaps = 256 - 256                    # the uniform total's trailing gap against the ragged scan region's
            uni = lib.lzh_decompress_temp_bytes(ZSTD, k * maxb, maxb)
            assert uni - split_bytes(maxb, k) == plan - rounding + gaps, (maxb, k, uni, split_bytes(maxb, k))


def test_debug_layout_regions_are_disjoint_and_inside_the_sizing_answer():
    for maxb in (SPLIT_MIN, 70000, 131072, 300000, MAX):
        for k in (0, 1, 9, 1000):
            rc, v = temp_layout(maxb, k)
            assert rc == OK
            total = v[15]
            assert total == split_bytes(maxb, k)
            regs = sorted((v[2 * i], v[2 * i + 1], REGIONS[i]) for i in range(7))
            end = 0
            for off, size, name in regs:
                assert off >= end, (maxb, k, name)             # (in order, no overlap)
                assert off % 256 == 0, (maxb, k, name)
                end = off + size
            assert end <= total
            by = {REGIONS[i]: (v[2 * i], v[2 * i + 1]) for i in range(7)}
            assert by["offsets"] == (0, 8 * (k + 1))            # where the one-wave call scans them to
            assert by["frames"][1] == k * v[14] and v[14] % 256 == 0
            assert by["dummy"][0] == by["frames"][0] + by["frames"][1]   # the kernels address both from `frames`
            assert by["states"][1] == 4 * k and by["njobs"][1] == 4
            assert by["jobs"][1] >= 64 * k * ((maxb + 131071) // 131072)  # a Huffman job per block
    # a frame's area holds its sequence records, 8 bytes for every 4 bytes of output
    assert temp_layout(131072, 1)[1][14] >= 2 * 131072


def test_debug_layout_refuses_what_the_sizing_refuses():
    out = np.zeros(16, np.uint64)
    lib = L.lib()
    assert lib.lzh_debug_zstd_ragged_split_layout(SPLIT_MIN - 1, 4, out.ctypes.data) == EARG
    assert lib.lzh_debug_zstd_ragged_split_layout(MAX + 1, 4, out.ctypes.data) == EARG
    assert lib.lzh_debug_zstd_ragged_split_layout(65536, 4, None) == EARG


def test_python_mirror():
    """RaggedCodec's checks come before any torch call: no device needed."""
    for codec in ("lz4", "snappy"):
        with pytest.raises(ValueError):
            L.RaggedCodec(codec, 65536, 4, split_decode=True)
