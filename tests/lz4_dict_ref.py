"""The reference build's own LZ4 dictionary functions (oracle/_ref/libref.so exports lz4's public functions), bound
through ctypes: the checker of the dictionary calls (include/lzbench_hip.h 3d).

compress(): a fresh LZ4_stream_t per chunk, LZ4_loadDict on `dict || chunk` in one buffer, LZ4_compress_fast_continue
(prefix mode).  decompress(): LZ4_decompress_safe_usingDict with the dictionary in a buffer of its own, as the GPU
sees it.  A test that needs a symbol the library lacks skips with its name (need()); test_lz4_dict_ref.py asserts
that all six resolve, so that skip cannot hide."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

SYMBOLS = ("LZ4_createStream", "LZ4_loadDict", "LZ4_compress_fast_continue", "LZ4_freeStream", "LZ4_compressBound",
           "LZ4_decompress_safe_usingDict")
_P, _I = C.c_void_p, C.c_int
_SIGS = {
    "LZ4_createStream": (_P, []),
    "LZ4_loadDict": (_I, [_P, _P, _I]),
    "LZ4_compress_fast_continue": (_I, [_P, _P, _P, _I, _I, _I]),
    "LZ4_freeStream": (_I, [_P]),
    "LZ4_compressBound": (_I, [_I]),
    "LZ4_decompress_safe_usingDict": (_I, [_P, _P, _I, _I, _P, _I]),
    "LZ4_compress_fast": (_I, [_P, _P, _I, _I, _I]),
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


_cache = {}


def compress(dictionary: np.ndarray, chunk: np.ndarray, acc: int = 1) -> bytes:
    """What lz4 1.9.3 writes for `chunk` after LZ4_loadDict(dictionary), the dictionary directly before the chunk."""
    key = (dictionary.tobytes(), chunk.tobytes(), acc)
    if key not in _cache:
        L = lib()
        nd, n = len(dictionary), len(chunk)
        buf = np.concatenate([dictionary, chunk, np.zeros(16, np.uint8)]).astype(np.uint8)
        bound = L.LZ4_compressBound(n)
        dst = np.zeros(bound + 16, np.uint8)
        st = L.LZ4_createStream()
        assert st
        try:
            L.LZ4_loadDict(st, buf.ctypes.data, nd)
            r = L.LZ4_compress_fast_continue(st, buf.ctypes.data + nd, dst.ctypes.data, n, bound, acc)
        finally:
            L.LZ4_freeStream(st)
        assert r > 0
        _cache[key] = dst[:r].tobytes()
    return _cache[key]


def compress_plain(chunk: np.ndarray, acc: int = 1) -> bytes:
    """LZ4_compress_fast of the chunk alone."""
    L = lib()
    src = np.concatenate([chunk, np.zeros(16, np.uint8)]).astype(np.uint8)
    dst = np.zeros(L.LZ4_compressBound(len(chunk)) + 16, np.uint8)
    r = L.LZ4_compress_fast(src.ctypes.data, dst.ctypes.data, len(chunk), len(dst) - 16, acc)
    assert r > 0
    return dst[:r].tobytes()


def packed(dictionary: np.ndarray, chunk: np.ndarray, acc: int = 1) -> bytes:
    """compress() with the raw-store rule: a block as long as its chunk is the chunk itself."""
    b = compress(dictionary, chunk, acc)
    return chunk.tobytes() if len(b) == len(chunk) else b


def decompress(dictionary: np.ndarray, block: bytes, cap: int):
    """(status, bytes) of LZ4_decompress_safe_usingDict(block, dst, len(block), cap, dictionary, len(dictionary));
    dst starts as zeros (an offset of 0 reads them back)."""
    L = lib()
    src = np.frombuffer(block, np.uint8).copy() if len(block) else np.zeros(1, np.uint8)
    d = np.ascontiguousarray(dictionary)
    dst = np.zeros(cap + 64, np.uint8)
    r = L.LZ4_decompress_safe_usingDict(src.ctypes.data, dst.ctypes.data, len(block), cap, d.ctypes.data, len(d))
    return r, (dst[:r].tobytes() if r >= 0 else b"")
