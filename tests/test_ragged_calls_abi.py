"""CPU: the argument checks of every ragged async call (include/lzbench_hip.h 3b .. 3g), driven by the table of
lzbench_amd.ragged_calls.  One contract, the check order of ragged_compress / ragged_decompress in csrc/api.cpp:
an unsupported head or size is LZH_EARG; then an empty batch is LZH_OK; then a null pointer is LZH_EARG; then a batch
over the launch-grid limit is LZH_EARG; then a short temp is LZH_ESPACE.  All of it comes before any device call."""
import pytest

import lzbench_amd as L
from lzbench_amd.ragged_calls import RAGGED_CALLS
from ragged_fake import CALLS, EARG, ESPACE, OK, fake_call, grid_limit

LZ4, SNAPPY = L.LZH_CODEC_LZ4, L.LZH_CODEC_SNAPPY
MIB = 1 << 20
MAX = 16 * MIB
SPLIT_MIN = 16384                 # (the smallest max_chunk_bytes with a split decoder)
HUGE = 1 << 40


def cfg(maxb, **head):
    return dict(head, max_chunk_bytes=maxb)


# A supported configuration per family and direction: head values and a max_chunk_bytes (values a call's head does not
# name are not passed to it).  UNSUPPORTED: the same, refused by the head or by the size.
LZ = [cfg(m, codec=c, level=1) for c in (LZ4, SNAPPY) for m in (65536, MAX)]
LZ_BAD = ([cfg(65536, codec=c, level=1) for c in (L.LZH_CODEC_MEMCPY, L.LZH_CODEC_ZSTD, L.LZH_CODEC_LZ4F,
                                                    L.LZH_CODEC_NVLZ4, L.LZH_CODEC_ZSTD_DFAST)]
          + [cfg(MAX + 1, codec=c, level=1) for c in (LZ4, SNAPPY)])
ZSTD = [cfg(65536, level=1), cfg(300000, level=-5), cfg(131072, level=2), cfg(0, level=-1)]
ZSTD_BAD = [cfg(m, level=lv) for lv, m in [(0, 65536), (3, 65536), (2, 131073), (2, MIB), (19, 4096), (1, MAX + 1),
                                           (-1, MAX + 1), (2, MAX + 1)]]
ZSTD_DECODE = [cfg(m) for m in (65536, 300000, 131072, 0, SPLIT_MIN, SPLIT_MIN - 1)]
ZSTD_DECODE_BAD = [cfg(MAX + 1)]
DFAST = [cfg(m, level=3) for m in (65536, 300000, 0)]
DFAST_BAD = [cfg(m, level=lv) for lv, m in [(1, 65536), (2, 65536), (4, 65536), (-1, 65536), (0, 4096), (19, 4096),
                                            (3, MAX + 1), (1, MAX + 1)]]
LZ4_DICT = [cfg(4096, level=1, dict_bytes=4096), cfg(4 * MIB, level=1, dict_bytes=8), cfg(0, level=1, dict_bytes=65536)]
LZ4_DICT_BAD = [cfg(4096, level=1, dict_bytes=nd) for nd in (0, 7, 65537)] + [cfg(4 * MIB + 1, level=1, dict_bytes=4096)]
ZSTD_DICT = [cfg(4096, level=1, dict_bytes=4096), cfg(131072, level=1, dict_bytes=8), cfg(0, level=1, dict_bytes=131072)]
ZSTD_DICT_SIZES_BAD = [cfg(4096, level=1, dict_bytes=7), cfg(131073, level=1, dict_bytes=4096)]
ZSTD_DICT_BAD = ZSTD_DICT_SIZES_BAD + [cfg(4096, level=lv, dict_bytes=4096) for lv in (2, 3)]
# (family, compress) -> (supported, unsupported); the decoders of zstd_dict take no level
CONFIGS = {("lz", True): (LZ, LZ_BAD), ("lz", False): (LZ, LZ_BAD),
           ("zstd", True): (ZSTD, ZSTD_BAD), ("zstd", False): (ZSTD_DECODE, ZSTD_DECODE_BAD),
           ("zstd_dfast", True): (DFAST, DFAST_BAD),
           ("lz4_dict", True): (LZ4_DICT, LZ4_DICT_BAD), ("lz4_dict", False): (LZ4_DICT, LZ4_DICT_BAD),
           ("zstd_dict", True): (ZSTD_DICT, ZSTD_DICT_BAD), ("zstd_dict", False): (ZSTD_DICT, ZSTD_DICT_SIZES_BAD)}


def cases(which):
    for r in RAGGED_CALLS:
        for c in CONFIGS[r.family, r.compress][which]:
            yield pytest.param(r.symbol, c, id=r.symbol[4:-6] + "-" + "-".join(str(c[n]) for n in r.sizing.head[:2] + (
                "max_chunk_bytes",) if n in c))


def test_every_call_of_the_table_has_configurations():
    assert len(RAGGED_CALLS) == 13 == len(CALLS)
    for r in RAGGED_CALLS:
        good, bad = CONFIGS[r.family, r.compress]
        assert good and bad, r.symbol


@pytest.mark.parametrize("symbol,c", cases(0))
def test_check_order(symbol, c):
    rec, lib, k, maxb = CALLS[symbol], L.lib(), 4, c["max_chunk_bytes"]
    for total in (4 * maxb, 2 * maxb + 17):
        v = dict(c, total=total, nchunks=k)
        need = rec.sizing(lib, **v)
        assert need > 0
        roomy = rec.roomy(lib, **v) if rec.roomy else 0       # (the split decoder's temp: the same checks with it)
        assert roomy == 0 or roomy >= need
        temps = sorted({0, need - 1, need, roomy or need, HUGE})
        for temp in temps:
            # an empty batch before the null pointers
            assert fake_call(symbol, "all", **dict(v, nchunks=0), temp_bytes=temp) == OK, temp
            # a null pointer before the launch grid and before temp_bytes
            for name in rec.required_pointers:
                assert fake_call(symbol, [name], **v, temp_bytes=temp) == EARG, (name, temp)
                assert fake_call(symbol, [name], **dict(v, nchunks=1 << 31), temp_bytes=temp) == EARG, (name, temp)
                assert fake_call(symbol, (name,) + rec.nullable, **v, temp_bytes=temp) == EARG, (name, temp)
            # the launch grid before temp_bytes
            limit = grid_limit(rec, maxb)
            for n in (limit + 1, 1 << 24, 1 << 31):
                if n > limit:
                    assert fake_call(symbol, **dict(v, nchunks=n), temp_bytes=temp) == EARG, (n, temp)
        assert fake_call(symbol, **dict(v, nchunks=limit), temp_bytes=0) == ESPACE     # (the limit itself: accepted)
        # temp_bytes one below the sizing answer -- for the decoders with a split decoder the one-wave answer: below the
        # larger one they fall back -- and a pointer that may be null does not change the verdict
        assert fake_call(symbol, **v, temp_bytes=need - 1) == ESPACE
        assert fake_call(symbol, **v, temp_bytes=0) == ESPACE
        assert fake_call(symbol, rec.nullable, **v, temp_bytes=need - 1) == ESPACE
        if "total" in rec.sizing.head and maxb:
            # a temp sized for a smaller promise
            for small, large in ((4 * maxb, 8 * maxb), (8 * maxb, 64 * maxb)):
                short = rec.sizing(lib, **dict(v, nchunks=64, total=small))
                assert fake_call(symbol, **dict(v, nchunks=64, total=large), temp_bytes=short) == ESPACE, (small, large)


@pytest.mark.parametrize("symbol,c", cases(1))
def test_unsupported_head_or_size_comes_first(symbol, c):
    rec, lib = CALLS[symbol], L.lib()
    v = dict(c, total=1 << 18, nchunks=4)
    assert rec.sizing(lib, **v) == 0
    assert rec.roomy is None or rec.roomy(lib, **v) == 0
    for temp in (0, HUGE):
        assert fake_call(symbol, **v, temp_bytes=temp) == EARG
        assert fake_call(symbol, "all", **dict(v, nchunks=0), temp_bytes=temp) == EARG      # (before the empty batch)
        for name in rec.required_pointers:
            assert fake_call(symbol, [name], **v, temp_bytes=temp) == EARG, name
