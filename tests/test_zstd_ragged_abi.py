"""CPU: the ragged zstd calls of include/lzbench_hip.h 3c without a device -- sizing functions, and that the
calls of 3b still refuse zstd (the calls' own argument checks: tests/test_ragged_calls_abi.py)."""
import pytest

import lzbench_amd as L

ZSTD = L.LZH_CODEC_ZSTD
EARG = -1
FAKE = 0x1000   # a non-null "device pointer": the checks under test return before anything reads it
MAX = 16 << 20
# (level, largest max_chunk_bytes it is accepted for)
GOOD = [(1, MAX), (-1, MAX), (-5, MAX), (2, 131072)]
# ZSTD_getParams size classes (16 KiB, 128 KiB, 256 KiB), block boundaries, the limit
SIZES = [0, 1, 6, 7, 63, 64, 255, 1024, 4099, 16384, 16385, 65536, 131072, 131073, 200000, 262144, 262145, 300000,
         1 << 20, (1 << 20) + 1, MAX]


@pytest.mark.parametrize("level,top", GOOD)
def test_sizing_is_nonzero_for_supported_levels(level, top):
    lib = L.lib()
    for maxb in [s for s in SIZES if s <= top]:
        assert lib.lzh_level_supported(ZSTD, level, maxb) == 1
        for k in (0, 1, 4, 1000):
            ct = lib.lzh_zstd_ragged_compress_temp_bytes(level, maxb, k)
            assert ct > 0, (maxb, k)
            # a staging slot and a scratch area per chunk
            assert ct >= k * lib.lzh_stage_stride(ZSTD, max(maxb, 1))
            assert lib.lzh_zstd_ragged_decompress_temp_bytes(maxb, k) >= 8 * (k + 1)


@pytest.mark.parametrize("level,maxb", [(0, 65536), (3, 65536), (2, 131073), (2, 1 << 20), (19, 4096), (1, MAX + 1),
                                        (-1, MAX + 1), (2, MAX + 1)])
def test_unsupported_level_or_size(level, maxb):
    lib = L.lib()
    assert lib.lzh_zstd_ragged_compress_temp_bytes(level, maxb, 4) == 0
    if maxb > MAX:
        assert lib.lzh_zstd_ragged_decompress_temp_bytes(maxb, 4) == 0
    else:   # (the decoder has no level: any frame of lzbench's shape)
        assert lib.lzh_zstd_ragged_decompress_temp_bytes(maxb, 4) > 0


@pytest.mark.parametrize("level,top", GOOD)
def test_sizing_functions_are_monotone(level, top):
    lib = L.lib()
    sizes = [s for s in SIZES if s <= top]
    counts = (0, 1, 2, 255, 256, 257, 1000, 16384)
    for f in (lambda m, k: lib.lzh_zstd_ragged_compress_temp_bytes(level, m, k), lib.lzh_zstd_ragged_decompress_temp_bytes):
        for maxb in sizes:
            prev = 0
            for k in counts:
                v = f(maxb, k)
                assert v >= prev and v > 0, (maxb, k)
                prev = v
        for k in counts:
            prev = 0
            for maxb in sizes:
                v = f(maxb, k)
                assert v >= prev, (maxb, k)
                prev = v


def test_max_packed_bytes():
    lib = L.lib()
    for k in (0, 1, 16, 1000):
        prev = 0
        for n in (0, 1, 64, 255, 256, 65536, 1 << 20, 1 << 30):
            v = lib.lzh_zstd_ragged_max_packed_bytes(n, k)
            assert v >= prev and v >= n
            prev = v
    for n in (0, 1, 65536, 1 << 20):
        prev = 0
        for k in (0, 1, 2, 1000):
            v = lib.lzh_zstd_ragged_max_packed_bytes(n, k)
            assert v >= prev
            prev = v
        assert lib.lzh_zstd_ragged_max_packed_bytes(n, 1) >= lib.lzh_max_packed_bytes(ZSTD, n, max(n, 1))
    # zstd expands small chunks (1..64 bytes become size + 9, an empty one 9): the LZ4 formula's one byte per
    # chunk would not hold them; the bound is the sum of the per-chunk bounds the staging slots are sized for
    for size in (0, 1, 6, 7, 64):
        assert lib.lzh_zstd_ragged_max_packed_bytes(1000 * size, 1000) >= 1000 * (size + 9)
    def zbound(n):   # ZSTD_COMPRESSBOUND (zstd.h), the bound a staging slot holds: stride = bound + 16, 256-aligned
        return n + (n >> 8) + (((128 << 10) - n) >> 11 if n < (128 << 10) else 0)

    for sizes in ([0, 1, 64, 65, 4099, 131072, 131073, 300000], [1 << 20] * 3 + [5], [7] * 100, [255] * 256):
        for s in set(sizes):
            assert lib.lzh_stage_stride(ZSTD, s) == (zbound(s) + 16 + 255) // 256 * 256
        assert lib.lzh_zstd_ragged_max_packed_bytes(sum(sizes), len(sizes)) >= sum(zbound(s) for s in sizes)


def test_the_calls_of_3b_still_refuse_zstd():
    lib = L.lib()
    assert lib.lzh_ragged_compress_temp_bytes(ZSTD, 65536, 4) == 0
    assert lib.lzh_ragged_decompress_temp_bytes(ZSTD, 65536, 4) == 0
    assert lib.lzh_ragged_compact_compress_temp_bytes(ZSTD, 1 << 20, 65536, 4) == 0
    assert lib.lzh_compress_ragged_async(ZSTD, 1, FAKE, FAKE, 4, 65536, FAKE, 1 << 20, FAKE, FAKE, FAKE, 1 << 30,
                                         None) == EARG
    assert lib.lzh_decompress_ragged_async(ZSTD, FAKE, 1 << 20, FAKE, None, FAKE, FAKE, 4, 65536, FAKE, FAKE, 1 << 30,
                                           None) == EARG
    assert lib.lzh_compress_ragged_compact_async(ZSTD, 1, FAKE, FAKE, 4, 65536, 1 << 20, FAKE, 1 << 20, FAKE, FAKE,
                                                 FAKE, 1 << 30, None) == EARG


def test_python_mirror_refuses_what_the_library_refuses():
    """RaggedCodec's checks come before any torch call: no device needed."""
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd", 65536, 4, level=1, compact=True)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd", 65536, 4, level=3)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd", 131073, 4, level=2)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd_fast", (16 << 20) + 1, 4, level=-1)
