"""LZH_CODEC_ZSTD_DFAST (zstd level 3, include/lzbench_hip.h) on the CPU: the level predicate, the sizing answers and
the argument checks of the calls, all host arithmetic that runs before any device call."""
import ctypes as C

import pytest

import lzbench_amd as L

DF, ZS = L.LZH_CODEC_ZSTD_DFAST, L.LZH_CODEC_ZSTD
MIB = 1 << 20
SIZES = (1, 7, 64, 1023, 16384, 16385, 65536, 131072, 131073, 262144, 262145, MIB, 4 * MIB, 16 * MIB)
FAKE = 0x10000     # a non-null pointer for calls that must return before they touch anything


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def test_codec_id_and_tables():
    assert DF == 6 and L.CODECS["zstd_dfast"] == 6 and "zstd_dfast" in L._LEVELED
    d = L.find_compressor("zstd_dfast")
    assert (d.name, d.first_level, d.last_level) == ("hip_zstd_dfast", 3, 3)
    assert d.compress == "lzbench_hip_zstd_dfast_compress" and d.decompress == "lzbench_hip_zstd_decompress"
    assert d.init == "lzbench_hip_zstd_dfast_init"


def test_level_supported(lib):
    for n in SIZES:
        assert lib.lzh_level_supported(DF, 3, n) == 1, n
        for level in (0, 1, 2, 4, 5, -1, 22):
            assert lib.lzh_level_supported(DF, level, n) == 0, (level, n)
        assert lib.lzh_level_supported(ZS, 3, n) == 0, n       # LZH_CODEC_ZSTD keeps refusing level 3


def test_sizing_answers(lib):
    for chunk in SIZES:
        assert lib.lzh_stage_stride(DF, chunk) == lib.lzh_stage_stride(ZS, chunk)
        for n in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 40 * MIB):
            assert lib.lzh_max_packed_bytes(DF, n, chunk) == lib.lzh_max_packed_bytes(ZS, n, chunk)
            t = lib.lzh_compress_temp_bytes(DF, n, chunk)
            assert t > 0 and t >= lib.lzh_compress_temp_bytes(ZS, n, chunk), (n, chunk)
            assert lib.lzh_decompress_temp_bytes(DF, n, chunk) == lib.lzh_decompress_temp_bytes(ZS, n, chunk)
    # non-decreasing in n and in chunk_size (the same number of chunks)
    ns = (0, 1, 100, 65536, 65537, 300_000, MIB, 5 * MIB + 3, 64 * MIB)
    for chunk in SIZES:
        t = [lib.lzh_compress_temp_bytes(DF, n, chunk) for n in ns]
        assert t == sorted(t), chunk
    for k in (1, 3, 64):
        t = [lib.lzh_compress_temp_bytes(DF, k * chunk, chunk) for chunk in SIZES]
        assert t == sorted(t), k
    # the tables: 768 KiB a frame above 256 KiB chunks, 192 KiB at 16 KiB (two frames' difference: the stride)
    def stride(chunk):
        return lib.lzh_compress_temp_bytes(DF, 2 * chunk, chunk) - lib.lzh_compress_temp_bytes(DF, chunk, chunk) \
            - lib.lzh_stage_stride(DF, chunk)
    assert stride(16384) >= (192 << 10) and stride(MIB) >= (768 << 10)
    assert stride(MIB) == stride(262145) == stride(16 * MIB)    # one block size, one pair of tables
    assert stride(MIB) - stride(262144) == (256 << 10)          # hashLog 17 instead of 16


def compress(lib, codec=DF, level=3, d_in=FAKE, n=MIB, readable=None, chunk=131072, packed=FAKE, cap=None, cs=FAKE,
             offs=FAKE, temp=FAKE, tb=None):
    cap = lib.lzh_max_packed_bytes(codec, n, chunk) if cap is None else cap
    tb = lib.lzh_compress_temp_bytes(codec, n, chunk) if tb is None else tb
    return lib.lzh_compress_async(codec, level, d_in, n, n + 64 if readable is None else readable, chunk, packed, cap, cs,
                                  offs, temp, tb, None)


def test_compress_checks_in_the_uniform_calls_order(lib):
    EARG, ESPACE = -1, -3
    # arguments first
    for kw in (dict(chunk=0), dict(packed=None), dict(cs=None), dict(offs=None), dict(d_in=None), dict(readable=5)):
        assert compress(lib, **kw, tb=0, cap=0, level=1) == EARG, kw
    # then the temp, then the packed capacity: before the level is looked at
    need = lib.lzh_compress_temp_bytes(DF, MIB, 131072)
    assert compress(lib, tb=need - 1, cap=0, level=1) == ESPACE
    assert compress(lib, temp=None, cap=0, level=1) == ESPACE
    assert compress(lib, cap=lib.lzh_max_packed_bytes(DF, MIB, 131072) - 1, level=1) == ESPACE
    # then the level and the chunk size
    for level in (0, 1, 2, 4, 5, -1, 22):
        assert compress(lib, level=level) == EARG, level
    assert compress(lib, n=64 * MIB, chunk=16 * MIB + 1) == EARG
    assert compress(lib, n=0x7fff0001, chunk=0x7fff0001) == EARG
    # LZH_CODEC_ZSTD at level 3: refused as before
    assert compress(lib, codec=ZS, level=3) == EARG


def test_other_entry_points_refuse_the_codec(lib):
    EARG = -1
    assert lib.lzh_compress_kernel_only(DF, 3, FAKE, MIB, MIB + 64, 131072, FAKE, FAKE, None) == EARG
    for mask in (1, 2, 3):
        assert lib.lzh_compress_kernel_stage(DF, 3, mask, FAKE, MIB, MIB + 64, 131072, FAKE, FAKE, None) == EARG
    assert lib.lzh_compress_finish_async(DF, FAKE, MIB, MIB + 64, 131072, FAKE, FAKE, FAKE, 1 << 40, FAKE, None) == EARG
    # the ragged calls (3b) and their temp sizing
    assert lib.lzh_ragged_compress_temp_bytes(DF, 65536, 8) == 0
    assert lib.lzh_ragged_decompress_temp_bytes(DF, 65536, 8) == 0
    assert lib.lzh_ragged_compact_compress_temp_bytes(DF, 8 * 65536, 65536, 8) == 0
    assert lib.lzh_compress_ragged_async(DF, 3, FAKE, FAKE, 8, 65536, FAKE, 1 << 30, FAKE, FAKE, FAKE, 1 << 40, None) == EARG
    assert lib.lzh_compress_ragged_compact_async(DF, 3, FAKE, FAKE, 8, 65536, 8 * 65536, FAKE, 1 << 30, FAKE, FAKE, FAKE,
                                                 1 << 40, None) == EARG
    assert lib.lzh_decompress_ragged_async(DF, FAKE, 1 << 20, FAKE, FAKE, FAKE, FAKE, 8, 65536, FAKE, FAKE, 1 << 40,
                                           None) == EARG
    out = (C.c_uint64 * 4)()
    assert lib.lzh_debug_ragged_compact_regions(DF, 8 * 65536, 65536, 8, out) == EARG
    # the ragged zstd calls (3c) take a level, not a codec: level 3 stays refused there
    assert lib.lzh_zstd_ragged_compress_temp_bytes(3, 65536, 8) == 0
    assert lib.lzh_zstd_ragged_compact_compress_temp_bytes(3, 8 * 65536, 65536, 8) == 0
    assert lib.lzh_zstd_compress_ragged_async(3, FAKE, FAKE, 8, 65536, FAKE, 1 << 30, FAKE, FAKE, FAKE, 1 << 40, None) == EARG


def test_decompress_call_takes_the_codec(lib):
    # n == 0 returns LZH_OK after the argument checks, as for LZH_CODEC_ZSTD; an unknown id stays an error
    assert lib.lzh_decompress_async(DF, FAKE, 64, FAKE, None, 0, 131072, FAKE, FAKE, None, 0, None) == 0
    assert lib.lzh_decompress_async(ZS, FAKE, 64, FAKE, None, 0, 131072, FAKE, FAKE, None, 0, None) == 0
    assert lib.lzh_decompress_async(7, FAKE, 64, FAKE, None, 0, 131072, FAKE, FAKE, None, 0, None) == -1
