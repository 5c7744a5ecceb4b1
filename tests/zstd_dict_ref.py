"""The reference build's own zstd dictionary functions (oracle/_ref/libref.so exports zstd's public functions), bound
through ctypes: the checker of the zstd dictionary calls (include/lzbench_hip.h 3f).

compress(): a fresh ZSTD_CCtx per chunk and ZSTD_compress_usingDict with the dictionary in a buffer of its own -- the
helper asserts that the chunk does not start where the dictionary ends, because the reference then runs its prefix
parser and writes other bytes (compress_adjacent() does that on purpose; test_zstd_dict_ref.py pins the difference).
decompress(): ZSTD_decompress_usingDict.  A test that needs a symbol the library lacks skips with its name (need());
test_zstd_dict_ref.py asserts that all of them resolve, so that skip cannot hide."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import zstd_census

SYMBOLS = ("ZSTD_createCCtx", "ZSTD_freeCCtx", "ZSTD_compress_usingDict", "ZSTD_createDCtx", "ZSTD_freeDCtx",
           "ZSTD_decompress_usingDict", "ZSTD_compressCCtx", "ZSTD_getParams", "ZSTD_compressBound", "ZSTD_isError")
_P, _I, _SZ = C.c_void_p, C.c_int, C.c_size_t


class CParams(C.Structure):
    _fields_ = [(n, C.c_uint) for n in ("windowLog", "chainLog", "hashLog", "searchLog", "minMatch", "targetLength",
                                        "strategy")]


class Params(C.Structure):
    _fields_ = [("cParams", CParams), ("contentSizeFlag", _I), ("checksumFlag", _I), ("noDictIDFlag", _I)]


_SIGS = {
    "ZSTD_createCCtx": (_P, []),
    "ZSTD_freeCCtx": (_SZ, [_P]),
    "ZSTD_compress_usingDict": (_SZ, [_P, _P, _SZ, _P, _SZ, _P, _SZ, _I]),
    "ZSTD_createDCtx": (_P, []),
    "ZSTD_freeDCtx": (_SZ, [_P]),
    "ZSTD_decompress_usingDict": (_SZ, [_P, _P, _SZ, _P, _SZ, _P, _SZ]),
    "ZSTD_compressCCtx": (_SZ, [_P, _P, _SZ, _P, _SZ, _I]),
    "ZSTD_getParams": (Params, [_I, C.c_ulonglong, _SZ]),
    "ZSTD_compressBound": (_SZ, [_SZ]),
    "ZSTD_isError": (C.c_uint, [_SZ]),
}
_lib = None


def missing():
    """Names of the needed symbols that oracle/_ref/libref.so lacks (all of them without the library)."""
    if not O.have_ref():
        return list(SYMBOLS)
    L = C.CDLL(O.REF_PATH)
    return [s for s in SYMBOLS if not hasattr(L, s)]


def need():
    m = missing()
    if m:
        pytest.skip("reference build lacks " + ", ".join(m))


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(O.REF_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def cparams(level: int, n: int, dict_bytes: int):
    """(windowLog, hashLog, minMatch, targetLength, strategy) of ZSTD_getParams(level, n, dict_bytes)"""
    c = lib().ZSTD_getParams(level, n, dict_bytes).cParams
    return c.windowLog, c.hashLog, c.minMatch, c.targetLength, c.strategy


_cache = {}


def _compress(dictionary, chunk, level, adjacent):
    L = lib()
    nd, n = len(dictionary), len(chunk)
    if adjacent:
        buf = np.concatenate([dictionary, chunk, np.zeros(16, np.uint8)]).astype(np.uint8)
        dp, sp = buf.ctypes.data, buf.ctypes.data + nd
    else:
        # one allocation, the chunk first and a gap before the dictionary: the chunk cannot start where the
        # dictionary ends
        buf = np.concatenate([chunk, np.zeros(64, np.uint8), dictionary, np.zeros(16, np.uint8)]).astype(np.uint8)
        sp, dp = buf.ctypes.data, buf.ctypes.data + n + 64
        assert sp != dp + nd, "the chunk starts where the dictionary ends: the reference would run its prefix parser"
    bound = L.ZSTD_compressBound(n)
    dst = np.zeros(bound + 16, np.uint8)
    cctx = L.ZSTD_createCCtx()
    assert cctx
    try:
        r = L.ZSTD_compress_usingDict(cctx, dst.ctypes.data, bound, sp, n, dp, nd, level)
    finally:
        L.ZSTD_freeCCtx(cctx)
    assert not L.ZSTD_isError(r)
    return dst[:r].tobytes()


def compress(dictionary: np.ndarray, chunk: np.ndarray, level: int = 1) -> bytes:
    """What zstd 1.5.2 writes for ZSTD_compress_usingDict(chunk, dictionary, level), the dictionary in a buffer of
    its own (the extDict parser)."""
    key = (dictionary.tobytes(), chunk.tobytes(), level)
    if key not in _cache:
        _cache[key] = _compress(dictionary, chunk, level, False)
    return _cache[key]


def compress_adjacent(dictionary: np.ndarray, chunk: np.ndarray, level: int = 1) -> bytes:
    """The same call with the dictionary directly before the chunk (the prefix parser): not what the GPU writes."""
    return _compress(dictionary, chunk, level, True)


def compress_plain(chunk: np.ndarray, level: int = 1) -> bytes:
    """ZSTD_compressCCtx of the chunk alone."""
    L = lib()
    src = np.concatenate([chunk, np.zeros(16, np.uint8)]).astype(np.uint8)
    bound = L.ZSTD_compressBound(len(chunk))
    dst = np.zeros(bound + 16, np.uint8)
    cctx = L.ZSTD_createCCtx()
    try:
        r = L.ZSTD_compressCCtx(cctx, dst.ctypes.data, bound, src.ctypes.data, len(chunk), level)
    finally:
        L.ZSTD_freeCCtx(cctx)
    assert not L.ZSTD_isError(r)
    return dst[:r].tobytes()


def _raw_rule(b: bytes, chunk: np.ndarray) -> bytes:
    return chunk.tobytes() if len(b) == len(chunk) else b


def packed(dictionary: np.ndarray, chunk: np.ndarray, level: int = 1) -> bytes:
    """compress() with the raw-store rule: a frame as long as its chunk is the chunk itself."""
    return _raw_rule(compress(dictionary, chunk, level), chunk)


def packed_plain(chunk: np.ndarray, level: int = 1) -> bytes:
    return _raw_rule(compress_plain(chunk, level), chunk)


def packed_batch(dictionary: np.ndarray, parts, level: int = 1, plain=False):
    """(packed, csizes) as the reference writes the batch, raw-store rule applied"""
    blocks = [packed_plain(p, level) if plain else packed(dictionary, p, level) for p in parts]
    cs = np.array([len(b) for b in blocks], np.int32)
    return np.frombuffer(b"".join(blocks), np.uint8), cs


def decompress(dictionary: np.ndarray, frame: bytes, cap: int):
    """(status, bytes) of ZSTD_decompress_usingDict(dst, cap, frame, dictionary): the decoded size, or -1 for an
    error code."""
    L = lib()
    src = np.frombuffer(frame, np.uint8).copy() if len(frame) else np.zeros(1, np.uint8)
    d = np.concatenate([dictionary, np.zeros(16, np.uint8)]).astype(np.uint8)
    dst = np.zeros(cap + 64, np.uint8)
    dctx = L.ZSTD_createDCtx()
    try:
        r = L.ZSTD_decompress_usingDict(dctx, dst.ctypes.data, cap, src.ctypes.data, len(frame), d.ctypes.data,
                                        len(dictionary))
    finally:
        L.ZSTD_freeDCtx(dctx)
    if L.ZSTD_isError(r):
        return -1, b""
    return int(r), dst[:r].tobytes()


def block_fields(frame: bytes):
    """(sequences, literals) of a frame's one compressed block, or None where the block is raw / RLE (zstd_census)."""
    _, blocks, _ = zstd_census.walk(frame)
    if len(blocks) != 1:
        return None
    regen, nseq = blocks[0]
    return nseq, regen
