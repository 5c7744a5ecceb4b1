"""CPU: sizing and the Python refusals of the zstd dictionary calls (include/lzbench_hip.h 3f; the order of the async
calls' argument checks: tests/test_ragged_calls_abi.py)."""
import ctypes as C

import pytest

import lzbench_amd as L
from ragged_fake import fake_call

LZH_OK, LZH_EARG, LZH_ESPACE = 0, -1, -3
LEVELS_OK, LEVELS_BAD = (1, -1, -2, -3, -4, -5), (0, 2, 3, 4, -6, 19)
DICTS_OK, DICTS_BAD = (8, 9, 4096, 112640, 131072), (0, 7, 131073, 1 << 20)
CHUNKS_OK, CHUNKS_BAD = (0, 1, 1000, 65536, 131072), (131073, 1 << 20)
COMPRESS, DECOMPRESS = "lzh_zstd_compress_ragged_dict_async", "lzh_zstd_decompress_ragged_dict_async"


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def test_sizing_is_zero_exactly_where_the_calls_refuse(lib):
    for level in LEVELS_OK + LEVELS_BAD:
        for nd in DICTS_OK + DICTS_BAD:
            for maxb in CHUNKS_OK + CHUNKS_BAD:
                sizes_ok = nd in DICTS_OK and maxb in CHUNKS_OK
                ok = level in LEVELS_OK and sizes_ok
                ct = lib.lzh_zstd_dict_compress_temp_bytes(level, nd, maxb, 4)
                dt = lib.lzh_zstd_dict_decompress_temp_bytes(nd, maxb, 4)
                assert (ct > 0) == ok and (dt > 0) == sizes_ok, (level, nd, maxb)
                # (nchunks == 0 comes after the argument check)
                v = dict(level=level, dict_bytes=nd, max_chunk_bytes=maxb, temp_bytes=1 << 40)
                assert fake_call(COMPRESS, nchunks=0, **v) == (LZH_OK if ok else LZH_EARG)
                assert fake_call(DECOMPRESS, nchunks=0, **v) == (LZH_OK if sizes_ok else LZH_EARG)
                assert fake_call(COMPRESS, nchunks=4, **dict(v, temp_bytes=0)) == (LZH_ESPACE if ok else LZH_EARG)


def test_sizing_is_monotone(lib):
    dicts = (8, 9, 63, 64, 100, 1000, 4095, 4096, 8191, 8192, 16384, 65536, 112640, 131072)
    chunks = (0, 1, 7, 64, 1000, 4096, 8192, 16384, 65536, 131072)
    ks = (0, 1, 2, 100, 4096)
    for f, head in ((lib.lzh_zstd_dict_compress_temp_bytes, (1,)), (lib.lzh_zstd_dict_decompress_temp_bytes, ())):
        v = {(d, c, k): f(*head, d, c, k) for d in dicts for c in chunks for k in ks}
        for (d, c, k), x in v.items():
            assert all(v[(d2, c2, k2)] >= x for d2 in dicts if d2 >= d for c2 in chunks if c2 >= c for k2 in ks if k2 >= k)
    # the same answer at every accepted level
    for level in LEVELS_OK:
        assert lib.lzh_zstd_dict_compress_temp_bytes(level, 65536, 1024, 4096) == \
               lib.lzh_zstd_dict_compress_temp_bytes(1, 65536, 1024, 4096)


def test_debug_calls_refuse_what_the_async_calls_refuse(lib):
    out = (C.c_uint32 * 5)()
    assert lib.lzh_debug_zstd_dict_params(2, 1000, 4096, out) == LZH_EARG
    assert lib.lzh_debug_zstd_dict_params(1, 1000, 7, out) == LZH_EARG
    assert lib.lzh_debug_zstd_dict_params(1, 131073, 4096, out) == LZH_EARG
    assert lib.lzh_debug_zstd_dict_params(1, 1000, 4096, None) == LZH_EARG
    assert lib.lzh_debug_zstd_dict_parse(1, None, 4096, None, 0, None, 0) == LZH_EARG


def test_ragged_codec_argument_errors():
    import torch
    d = torch.zeros(4096, dtype=torch.uint8)
    for kw in (dict(level=2), dict(level=3), dict(level=0), dict(level=1, compact_scratch=True),
               dict(level=1, split_decode=True), dict(level=1, compact=True)):
        with pytest.raises(ValueError):
            L.RaggedCodec("zstd", 4096, 4, dictionary=d, **kw)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd_dfast", 4096, 4, level=3, dictionary=d)
    for bad in (torch.zeros(7, dtype=torch.uint8), torch.zeros(131073, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            L.RaggedCodec("zstd", 4096, 4, level=1, dictionary=bad)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd_fast", 131073, 4, level=-1, dictionary=d)
    magic = torch.zeros(4096, dtype=torch.uint8)
    magic[:4] = torch.tensor([0x37, 0xA4, 0x30, 0xEC], dtype=torch.uint8)
    with pytest.raises(ValueError, match="magic"):
        L.RaggedCodec("zstd", 4096, 4, level=1, dictionary=magic)
