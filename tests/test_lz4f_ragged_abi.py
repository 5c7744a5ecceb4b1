"""CPU: sizing, the order of the argument checks and the Python refusals of the ragged LZ4 frame calls
(include/lzbench_hip.h 3i).  The calls run with made-up pointers through a small fake of this file's own
(tests/ragged_fake.py holds the 13 calls of 3b .. 3g): every check comes before the first device call."""
import ctypes as C

import numpy as np
import pytest

import lz4f_ragged_cases as R
import lzbench_amd as L
from lzbench_amd.ragged_calls import ARG_TYPES, COMPRESS, DECOMPRESS, MORE_CALLS, RAGGED_CALLS

OK, EARG, ESPACE = 0, -1, -3
FAKE, GRID_MAX, HUGE = 0x1000, 0x7fffffff, 1 << 40
MIB = 1 << 20
MAX = 16 * MIB
# levels the compress call takes: block-size id 0 | 4 .. 7, the three checksum / size flags, an acceleration
LEVELS_OK = (0, 4, 5, 6, 7, 0x10, 0x20, 0x40, 0x74, 0x304, 0xff07)
# a bad block-size id, bit 3, linked blocks, a negative level, one past the 16 bits
LEVELS_BAD = (1, 2, 3, 8, 0x0c, 0x80, 0x84, 0xB0, -1, 1 << 16)
CHUNKS_OK, CHUNKS_BAD = (0, 1, 4096, 65536, 65537, 300000, MAX), (MAX + 1, 1 << 30)
CREC, DREC = COMPRESS["lz4f", False], DECOMPRESS["lz4f", False]


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def block_bytes(level):
    bid = level & 7
    return 1 << (8 + 2 * (bid if bid else 4))


def compress_bpf(level, maxb):
    bs = max(min(block_bytes(level), maxb), 1)
    return bs, max((maxb + bs - 1) // bs, 1)


def decode_bpf(maxb):
    return max((maxb + 65535) // 65536, 1)


def grid_factor(rec, level, maxb):
    return compress_bpf(level, maxb)[1] if rec.compress else decode_bpf(maxb)


def fake_call(rec, null=(), **values):
    """rec with FAKE for every pointer but those named in null ("all": every pointer).  Arguments that would pass every
    check and launch on the made-up pointers are a mistake of the test: refused here."""
    lib = L.lib()
    pointers = [n for n in rec.names if ARG_TYPES[n] is C.c_void_p and n != "stream"]
    null = pointers if null == "all" else null
    assert set(null) <= set(pointers)
    v = dict({n: FAKE for n in pointers}, packed_cap=1 << 20, packed_readable=1 << 20, stream=None)
    v.update(values, **{n: None for n in null})
    need = rec.sizing(lib, **v)
    limit = GRID_MAX // grid_factor(rec, v.get("level", 0), v["max_chunk_bytes"]) if need else 0
    launches = need and 0 < v["nchunks"] <= limit and v["temp_bytes"] >= need and not set(null) & set(rec.required_pointers)
    assert not launches, "these arguments pass every check"
    return rec(lib, **v)


def test_the_rows_and_their_table():
    assert CREC.symbol == "lzh_lz4f_compress_ragged_async" and DREC.symbol == "lzh_lz4f_decompress_ragged_async"
    for rec in (CREC, DREC):
        assert rec in MORE_CALLS and rec not in RAGGED_CALLS
        assert rec.symbol in L.SIGNATURES and rec.sizing.symbol in L.SIGNATURES
    assert len(RAGGED_CALLS) == 13
    # the compress tail of lzh_compress_ragged_async after the level; the decode call without the codec
    assert CREC.names == ("level",) + COMPRESS["lz", False].names[2:]
    assert DREC.names == DECOMPRESS["lz", False].names[1:]
    assert DREC.nullable == ("offsets",) and "offsets" not in DREC.required_pointers
    assert "lzh_lz4f_ragged_max_packed_bytes" in L.SIGNATURES


def test_sizing_is_zero_exactly_where_the_calls_refuse(lib):
    for level in LEVELS_OK + LEVELS_BAD:
        supported = lib.lzh_level_supported(L.LZH_CODEC_LZ4F, level, 65536) == 1 and not level & L.LZ4F_LINKED
        assert supported == (level in LEVELS_OK), hex(level)
        for maxb in CHUNKS_OK + CHUNKS_BAD:
            ok = supported and maxb in CHUNKS_OK
            assert (lib.lzh_lz4f_ragged_compress_temp_bytes(level, maxb, 4) > 0) == ok, (hex(level), maxb)
            v = dict(level=level, max_chunk_bytes=maxb)
            # (nchunks == 0 comes after the argument check)
            assert fake_call(CREC, nchunks=0, temp_bytes=HUGE, **v) == (OK if ok else EARG)
            assert fake_call(CREC, nchunks=4, temp_bytes=0, **v) == (ESPACE if ok else EARG)
            assert fake_call(CREC, "all", nchunks=4, temp_bytes=HUGE, **v) == EARG
    for maxb in CHUNKS_OK + CHUNKS_BAD:
        ok = maxb in CHUNKS_OK
        assert (lib.lzh_lz4f_ragged_decompress_temp_bytes(maxb, 4) > 0) == ok, maxb
        assert fake_call(DREC, nchunks=0, temp_bytes=HUGE, max_chunk_bytes=maxb) == (OK if ok else EARG)
        assert fake_call(DREC, nchunks=4, temp_bytes=0, max_chunk_bytes=maxb) == (ESPACE if ok else EARG)
        assert fake_call(DREC, "all", nchunks=4, temp_bytes=HUGE, max_chunk_bytes=maxb) == EARG


def test_sizing_is_monotone(lib):
    chunks = (0, 1, 12, 13, 4095, 4096, 65535, 65536, 65537, 131072, 131073, 262143, 262144, 262145, 300000, MIB,
              MIB + 1, 4 * MIB, 4 * MIB + 1, MAX)
    ks = (0, 1, 2, 3, 100, 4096, 1 << 20)
    for name, f in [(hex(lv), lambda m, k, lv=lv: lib.lzh_lz4f_ragged_compress_temp_bytes(lv, m, k)) for lv in LEVELS_OK] \
            + [("decode", lib.lzh_lz4f_ragged_decompress_temp_bytes)]:
        v = np.array([[f(m, k) for k in ks] for m in chunks], dtype=np.uint64)
        assert (v > 0).all(), name
        assert (np.diff(v.astype(np.int64), axis=0) >= 0).all() and (np.diff(v.astype(np.int64), axis=1) >= 0).all(), name
    totals = (0, 1, 65535, 65536, 65537, MIB, 1 << 32)
    p = np.array([[lib.lzh_lz4f_ragged_max_packed_bytes(t, k) for k in ks] for t in totals], dtype=np.uint64).astype(np.int64)
    assert (np.diff(p, axis=0) >= 0).all() and (np.diff(p, axis=1) >= 0).all()


def _al(v, gap=0):
    return (v + 255) // 256 * 256 + gap


@pytest.mark.parametrize("level", [0, 4, 5, 6, 7, 0x74])
def test_compress_temp_is_the_layout_of_nchunks_times_bpf_blocks(lib, level):
    """Uniform slots: nb = nchunks * bpf blocks of bs bytes.  A block takes what the LZ4 ragged call's layout gives a
    chunk of bs bytes -- a staging slot, a record slot, an 8-byte record header (lzh_ragged_compress_temp_bytes: the same
    three regions) -- then a u32 in each of the two block arrays and 8 + 8 bytes of block table; every region is rounded
    up to 256 and four of the new ones are followed by 256 spare bytes."""
    for maxb in CHUNKS_OK:
        bs, bpf = compress_bpf(level, maxb)
        for k in (0, 1, 3, 100, 4096):
            nb = k * bpf
            blocks = lib.lzh_ragged_compress_temp_bytes(L.LZH_CODEC_LZ4, bs, nb)
            assert blocks > 0
            want = blocks + 2 * _al(4 * nb, 256) + _al(8 * nb) + _al(8 * nb, 256)
            assert lib.lzh_lz4f_ragged_compress_temp_bytes(level, maxb, k) == want, (hex(level), maxb, k)
    # the skewed batch of the header's text: one 16 MiB chunk among 4096 is paid for 4096 times
    assert lib.lzh_lz4f_ragged_compress_temp_bytes(4, MAX, 4096) > 4096 * MAX


def test_decompress_temp_is_offsets_descriptors_and_statuses(lib):
    for maxb in CHUNKS_OK:
        for k in (0, 1, 3, 100, 4096):
            nd = k * decode_bpf(maxb)
            want = _al(8 * (k + 1), 256) + _al(32 * nd) + _al(4 * nd) + _al(4 * k, 256)
            assert lib.lzh_lz4f_ragged_decompress_temp_bytes(maxb, k) == want, (maxb, k)


@pytest.mark.parametrize("rec,level,maxb", [(CREC, 4, 65536), (CREC, 0x74, 300000), (CREC, 7, MAX), (CREC, 5, 0),
                                            (CREC, 4, MAX), (DREC, 0, 65536), (DREC, 0, 300000), (DREC, 0, MAX),
                                            (DREC, 0, 0)],
                         ids=lambda v: v.symbol[4:-6] if hasattr(v, "symbol") else hex(v))
def test_check_order(lib, rec, level, maxb):
    """arguments, nchunks == 0, null pointers, the launch grid, LZH_ESPACE (the order of ragged_compress in api.cpp)"""
    v = dict(max_chunk_bytes=maxb, nchunks=4)
    if rec.compress:
        v["level"] = level
    need = rec.sizing(lib, **v)
    assert need > 0
    limit = GRID_MAX // grid_factor(rec, level, maxb)
    for temp in sorted({0, need - 1, need, HUGE}):
        # an empty batch before the null pointers
        assert fake_call(rec, "all", **dict(v, nchunks=0), temp_bytes=temp) == OK, temp
        # a null pointer before the launch grid and before temp_bytes
        for name in rec.required_pointers:
            assert fake_call(rec, [name], **v, temp_bytes=temp) == EARG, (name, temp)
            assert fake_call(rec, [name], **dict(v, nchunks=1 << 31), temp_bytes=temp) == EARG, (name, temp)
            assert fake_call(rec, (name,) + rec.nullable, **v, temp_bytes=temp) == EARG, (name, temp)
        # the launch grid before temp_bytes
        for n in (limit + 1, 1 << 31, 1 << 32):
            assert fake_call(rec, **dict(v, nchunks=n), temp_bytes=temp) == EARG, (n, temp)
    assert fake_call(rec, **dict(v, nchunks=limit), temp_bytes=0) == ESPACE      # (the limit itself: accepted)
    assert fake_call(rec, **v, temp_bytes=need - 1) == ESPACE
    assert fake_call(rec, **v, temp_bytes=0) == ESPACE
    assert fake_call(rec, rec.nullable, **v, temp_bytes=need - 1) == ESPACE    # (a pointer that may be null)
    # an unsupported level or size comes before everything
    bad = [dict(max_chunk_bytes=MAX + 1)] + ([dict(level=lv) for lv in (1, 8, 0x80, 0x84)] if rec.compress else [])
    for b in bad:
        for temp in (0, HUGE):
            assert fake_call(rec, "all", **dict(v, **b, nchunks=0), temp_bytes=temp) == EARG
            assert fake_call(rec, **dict(v, **b), temp_bytes=temp) == EARG


def test_max_packed_bytes_holds_the_oracles_frames(lib):
    """the sum of the oracle's frame sizes plus 8 per chunk, for incompressible chunks with every optional field on"""
    sizes = (0, 1, 65536, 65537)
    parts = [L.datagen("random", n, seed=40 + i) for i, n in enumerate(sizes)]
    frames = [len(R.frame(p, 0x70)) for p in parts]
    assert frames[0] == 15 and all(f > n for f, n in zip(frames, sizes))
    assert lib.lzh_lz4f_ragged_max_packed_bytes(sum(sizes), len(sizes)) >= sum(frames) + 8 * len(sizes)
    for i, n in enumerate(sizes):     # (and each alone, and many of one size)
        assert lib.lzh_lz4f_ragged_max_packed_bytes(n, 1) >= frames[i] + 8
        assert lib.lzh_lz4f_ragged_max_packed_bytes(100 * n, 100) >= 100 * (frames[i] + 8)


def test_3b_keeps_refusing_the_framed_codecs(lib):
    lz = COMPRESS["lz", False], COMPRESS["lz", True], DECOMPRESS["lz", False]
    for codec in (L.LZH_CODEC_LZ4F, L.LZH_CODEC_NVLZ4):
        for rec in lz:
            v = dict(codec=codec, level=0, max_chunk_bytes=65536, nchunks=4, total=1 << 18)
            assert rec.sizing(lib, **v) == 0
            pointers = {n: FAKE for n in rec.names if ARG_TYPES[n] is C.c_void_p and n != "stream"}
            args = dict(pointers, packed_cap=1 << 20, packed_readable=1 << 20, temp_bytes=HUGE, stream=None, **v)
            assert rec(lib, **args) == EARG
            assert rec(lib, **dict(args, nchunks=0)) == EARG
    assert not any("nvlz4" in r.symbol or "nvcomp" in r.symbol for r in RAGGED_CALLS + MORE_CALLS)


def test_ragged_codec_argument_errors(monkeypatch):
    import torch
    # every refusal comes before any torch device call
    monkeypatch.setattr(torch.cuda, "current_device", lambda: pytest.fail("a device call before the checks"))
    d = torch.zeros(4096, dtype=torch.uint8)
    for kw in (dict(compact=True), dict(compact_scratch=True), dict(split_decode=True), dict(compact_decode=True),
               dict(split_decode=True, compact_decode=True), dict(dictionary=d)):
        with pytest.raises(ValueError):
            L.RaggedCodec("lz4frame", 4096, 4, level=4, **kw)
    for level in (0x80, 0x84, 0xB0, L.LZ4F_LINKED | 7):
        with pytest.raises(ValueError, match="LINKED"):
            L.RaggedCodec("lz4frame", 4096, 4, level=level)
    for level in (1, 8):
        with pytest.raises(ValueError, match="not supported"):
            L.RaggedCodec("lz4frame", 4096, 4, level=level)
    with pytest.raises(ValueError, match="not supported"):
        L.RaggedCodec("lz4frame", MAX + 1, 4, level=4)
    with pytest.raises(ValueError):
        L.RaggedCodec("nvcomp_lz4", 4096, 4)
