"""CPU: the C-ABI of the LZ4 dictionary calls (include/lzbench_hip.h 3d) -- the sizing functions and RaggedCodec's
argument errors (the async calls' argument checks: tests/test_ragged_calls_abi.py)."""
import itertools

import pytest

import lzbench_amd as L

LZH_OK, LZH_EARG, LZH_ESPACE = 0, -1, -3
MIB = 1 << 20
DICTS = [8, 11, 4095, 65535, 65536]
MAXES = [0, 1, 256, 4096, 65547, 200000, 4 * MIB]
COUNTS = [0, 1, 4, 4096, 100000]


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def test_error_codes_are_the_headers(lib):
    import re, os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lzbench_hip.h")).read()
    codes = dict(re.findall(r"(LZH_OK|LZH_EARG|LZH_ESPACE) = (-?\d+)", h))
    assert {k: int(v) for k, v in codes.items()} == {"LZH_OK": LZH_OK, "LZH_EARG": LZH_EARG, "LZH_ESPACE": LZH_ESPACE}


def test_sizing_is_zero_exactly_for_the_refused_arguments(lib):
    for f in (lib.lzh_lz4_dict_compress_temp_bytes, lib.lzh_lz4_dict_decompress_temp_bytes):
        for nd in (0, 1, 7, 65537, 1 << 20):
            assert f(nd, 4096, 16) == 0
        assert f(4096, 4 * MIB + 1, 16) == 0 and f(4096, 16 * MIB, 16) == 0
        for nd, m, k in itertools.product(DICTS, MAXES, COUNTS):
            assert f(nd, m, k) > 0, (nd, m, k)


def test_sizing_is_monotone_and_within_the_bound(lib):
    for f in (lib.lzh_lz4_dict_compress_temp_bytes, lib.lzh_lz4_dict_decompress_temp_bytes):
        for args in itertools.product(DICTS, MAXES, COUNTS):
            v = f(*args)
            for axis, grid in enumerate((DICTS, MAXES, COUNTS)):
                for bigger in (g for g in grid if g > args[axis]):
                    up = list(args)
                    up[axis] = bigger
                    assert f(*up) >= v, (args, up)
    # compress: at most the plain LZ4 ragged call's temp + 64 KiB + 64 bytes a chunk (no dictionary copy per chunk)
    for nd, m, k in itertools.product(DICTS, MAXES, COUNTS):
        plain = lib.lzh_ragged_compress_temp_bytes(L.LZH_CODEC_LZ4, m, k)
        assert plain > 0
        assert lib.lzh_lz4_dict_compress_temp_bytes(nd, m, k) <= plain + 65536 + 64 * k, (nd, m, k)


def test_ragged_codec_argument_errors():
    import torch
    d = torch.zeros(4096, dtype=torch.uint8)
    for codec in ("snappy", "zstd", "lz4frame"):
        with pytest.raises(ValueError):
            L.RaggedCodec(codec, 4096, 4, dictionary=d)
    with pytest.raises(ValueError):
        L.RaggedCodec("lz4", 4096, 4, dictionary=d, compact=True)
    for bad in (torch.zeros(7, dtype=torch.uint8), torch.zeros(65537, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            L.RaggedCodec("lz4", 4096, 4, dictionary=bad)
    with pytest.raises(ValueError):
        L.RaggedCodec("lz4", 4 * MIB + 1, 4, dictionary=d)
