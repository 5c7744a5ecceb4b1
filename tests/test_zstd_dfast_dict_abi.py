"""CPU: sizing, the order of the argument checks and the Python refusals of the zstd level-3 dictionary call
(include/lzbench_hip.h 3h).  The call runs with made-up pointers through a small fake of this file's own
(tests/ragged_fake.py holds the 13 calls of 3b .. 3g): every check comes before the first device call."""
import ctypes as C

import pytest

import lzbench_amd as L
from lzbench_amd.ragged_calls import ARG_TYPES, COMPRESS, DECOMPRESS, MORE_CALLS, RAGGED_CALLS

OK, EARG, ESPACE = 0, -1, -3
FAKE, GRID_MAX, HUGE = 0x1000, 0x7fffffff, 1 << 40
LEVELS_OK, LEVELS_BAD = (3,), (0, 1, 2, 4, -1, 19)
DICTS_OK, DICTS_BAD = (8, 9, 4096, 112640, 131072), (0, 7, 131073)
CHUNKS_OK, CHUNKS_BAD = (0, 1, 1000, 131072), (131073, 1 << 20)
REC = COMPRESS["zstd_dfast_dict", False]
POINTERS = [n for n in REC.names if ARG_TYPES[n] is C.c_void_p and n != "stream"]


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def fake_call(null=(), **values):
    """The call with FAKE for every pointer but those named in null ("all": every pointer).  Arguments that would pass
    every check and launch on the made-up pointers are a mistake of the test: refused here."""
    lib = L.lib()
    null = POINTERS if null == "all" else null
    assert set(null) <= set(POINTERS)
    v = dict({n: FAKE for n in POINTERS}, packed_cap=1 << 20, stream=None)
    v.update(values, **{n: None for n in null})
    need = REC.sizing(lib, **v)
    launches = need and 0 < v["nchunks"] <= GRID_MAX and v["temp_bytes"] >= need and not null
    assert not launches, "these arguments pass every check"
    return REC(lib, **v)


def test_the_row_and_its_table():
    assert REC.symbol == "lzh_zstd_dfast_compress_ragged_dict_async" and REC in MORE_CALLS and REC not in RAGGED_CALLS
    assert REC.names == COMPRESS["zstd_dict", False].names, "3f's arguments"
    assert REC.required_pointers == tuple(POINTERS) and "dict" in POINTERS
    assert ("zstd_dfast_dict", False) not in DECOMPRESS, "the frames decode through 3f's row"
    assert REC.symbol in L.SIGNATURES and REC.sizing.symbol in L.SIGNATURES


def test_sizing_is_zero_exactly_where_the_call_refuses(lib):
    for level in LEVELS_OK + LEVELS_BAD:
        for nd in DICTS_OK + DICTS_BAD:
            for maxb in CHUNKS_OK + CHUNKS_BAD:
                ok = level in LEVELS_OK and nd in DICTS_OK and maxb in CHUNKS_OK
                ct = lib.lzh_zstd_dfast_dict_compress_temp_bytes(level, nd, maxb, 4)
                assert (ct > 0) == ok, (level, nd, maxb)
                v = dict(level=level, dict_bytes=nd, max_chunk_bytes=maxb)
                # (nchunks == 0 comes after the argument check)
                assert fake_call(nchunks=0, temp_bytes=HUGE, **v) == (OK if ok else EARG)
                assert fake_call(nchunks=4, temp_bytes=0, **v) == (ESPACE if ok else EARG)
                assert fake_call("all", nchunks=4, temp_bytes=HUGE, **v) == EARG


def test_sizing_is_monotone(lib):
    dicts = (8, 9, 63, 64, 100, 1000, 4095, 4096, 8191, 8192, 16384, 32768, 65536, 112640, 131072)
    chunks = (0, 1, 7, 64, 1000, 4096, 8192, 16384, 65536, 131072)
    ks = (0, 1, 2, 100, 4096)
    f = lib.lzh_zstd_dfast_dict_compress_temp_bytes
    v = {(d, c, k): f(3, d, c, k) for d in dicts for c in chunks for k in ks}
    for (d, c, k), x in v.items():
        assert x > 0
        assert all(v[(d2, c2, k2)] >= x for d2 in dicts if d2 >= d for c2 in chunks if c2 >= c for k2 in ks if k2 >= k)


@pytest.mark.parametrize("nd,maxb", [(4096, 4096), (8, 131072), (131072, 0)])
def test_check_order(lib, nd, maxb):
    """arguments, nchunks == 0, null pointers, the launch grid, LZH_ESPACE (tests/test_ragged_calls_abi.py's order)"""
    v = dict(level=3, dict_bytes=nd, max_chunk_bytes=maxb, nchunks=4)
    need = REC.sizing(lib, **v)
    assert need > 0
    for temp in sorted({0, need - 1, need, HUGE}):
        # an empty batch before the null pointers
        assert fake_call("all", **dict(v, nchunks=0), temp_bytes=temp) == OK, temp
        # a null pointer before the launch grid and before temp_bytes
        for name in POINTERS:
            assert fake_call([name], **v, temp_bytes=temp) == EARG, (name, temp)
            assert fake_call([name], **dict(v, nchunks=1 << 31), temp_bytes=temp) == EARG, (name, temp)
        # the launch grid before temp_bytes
        for n in (GRID_MAX + 1, 1 << 32):
            assert fake_call(**dict(v, nchunks=n), temp_bytes=temp) == EARG, (n, temp)
    assert fake_call(**dict(v, nchunks=GRID_MAX), temp_bytes=0) == ESPACE      # (the limit itself: accepted)
    assert fake_call(**v, temp_bytes=need - 1) == ESPACE
    assert fake_call(**v, temp_bytes=0) == ESPACE
    # an unsupported head comes before everything
    for bad in (dict(level=1), dict(dict_bytes=7), dict(max_chunk_bytes=131073)):
        assert fake_call("all", **dict(v, **bad, nchunks=0), temp_bytes=HUGE) == EARG


def test_the_other_calls_keep_their_answers(lib):
    """3f keeps refusing level 3, the calls of 3e keep having no dictionary argument"""
    assert lib.lzh_zstd_dict_compress_temp_bytes(3, 4096, 4096, 4) == 0
    assert "dict" not in COMPRESS["zstd_dfast", False].names and "dict" not in COMPRESS["zstd_dfast", True].names
    assert len(RAGGED_CALLS) == 13


def test_debug_calls_refuse_what_the_async_call_refuses(lib):
    out = (C.c_uint32 * 5)()
    for level in LEVELS_BAD:
        assert lib.lzh_debug_zstd_dfast_dict_params(level, 1000, 4096, out) == EARG
        assert lib.lzh_debug_zstd_dfast_dict_parse(level, None, 4096, None, 0, None, 0, None) == EARG
    for nd in DICTS_BAD:
        assert lib.lzh_debug_zstd_dfast_dict_params(3, 1000, nd, out) == EARG
    for n in CHUNKS_BAD:
        assert lib.lzh_debug_zstd_dfast_dict_params(3, n, 4096, out) == EARG
    assert lib.lzh_debug_zstd_dfast_dict_params(3, 1000, 4096, None) == EARG
    assert lib.lzh_debug_zstd_dfast_dict_params(3, 1000, 4096, out) == OK
    assert lib.lzh_debug_zstd_dfast_dict_parse(3, None, 4096, None, 0, None, 0, None) == EARG
    buf = (C.c_uint8 * (4096 + 16))()
    assert lib.lzh_debug_zstd_dfast_dict_parse(3, buf, 4096, None, 10, None, 0, None) == EARG
    assert lib.lzh_debug_zstd_dfast_dict_parse(3, buf, 7, buf, 10, None, 0, None) == EARG
    assert lib.lzh_debug_zstd_dfast_dict_parse(3, buf, 4096, buf, 131073, None, 0, None) == EARG
    assert lib.lzh_debug_zstd_dfast_dict_parse(3, buf, 4096, None, 0, None, 0, None) == 0


def test_ragged_codec_argument_errors(monkeypatch):
    import torch
    # every refusal comes before any torch device call
    monkeypatch.setattr(torch.cuda, "current_device", lambda: pytest.fail("a device call before the checks"))
    d = torch.zeros(4096, dtype=torch.uint8)
    with pytest.raises(ValueError, match="dictionary"):
        L.RaggedCodec("zstd_dfast_dict", 4096, 4, level=3)
    for level in (0, 1, 2, 4, -1, 19):
        with pytest.raises(ValueError, match="level"):
            L.RaggedCodec("zstd_dfast_dict", 4096, 4, level=level, dictionary=d)
    for kw in (dict(compact_scratch=True), dict(split_decode=True), dict(split_decode=True, compact_decode=True),
               dict(compact_decode=True), dict(compact=True)):
        with pytest.raises(ValueError):
            L.RaggedCodec("zstd_dfast_dict", 4096, 4, level=3, dictionary=d, **kw)
    magic = torch.zeros(4096, dtype=torch.uint8)
    magic[:4] = torch.tensor([0x37, 0xA4, 0x30, 0xEC], dtype=torch.uint8)
    with pytest.raises(ValueError, match="magic"):
        L.RaggedCodec("zstd_dfast_dict", 4096, 4, level=3, dictionary=magic)
    for bad in (torch.zeros(7, dtype=torch.uint8), torch.zeros(131073, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            L.RaggedCodec("zstd_dfast_dict", 4096, 4, level=3, dictionary=bad)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd_dfast_dict", 131073, 4, level=3, dictionary=d)
    # the older spellings keep raising
    for name in ("zstd", "zstd_dfast"):
        with pytest.raises(ValueError):
            L.RaggedCodec(name, 4096, 4, level=3, dictionary=d)


def test_the_name_belongs_to_ragged_codec_alone():
    assert "zstd_dfast_dict" not in L.CODECS
    with pytest.raises((KeyError, ValueError)):
        L.DeviceCodec("zstd_dfast_dict", 1 << 20, 65536)
    with pytest.raises((KeyError, ValueError, LookupError)):
        L.find_compressor("zstd_dfast_dict")
    assert not any("dfast_dict" in c.name for c in L.COMP_DESC)
