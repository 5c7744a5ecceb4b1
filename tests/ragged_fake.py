"""The ragged async calls of lzbench_amd.ragged_calls with made-up device pointers, for the CPU tests of their
argument checks: every check comes before the first device call, so nothing reads the pointers."""
import lzbench_amd as L
from lzbench_amd.ragged_calls import ARG_TYPES, RAGGED_CALLS

OK, EARG, ESPACE = 0, -1, -3          # (include/lzbench_hip.h)
FAKE = 0x1000                          # a non-null "device pointer"
GRID_MAX = 0x7fffffff                  # (api.cpp: nchunks * grid_factor above it is refused)
CALLS = {r.symbol: r for r in RAGGED_CALLS}


def grid_limit(rec, max_chunk_bytes):
    """the largest nchunks whose launch grids the call accepts"""
    return GRID_MAX // rec.grid_factor(max_chunk_bytes)


def fake_call(symbol, null=(), **values):
    """The call `symbol`: its head, nchunks, max_chunk_bytes, temp_bytes (and total) from values, FAKE for every
    pointer but those named in null (null="all": every pointer).  A call that would pass every check and launch on
    the made-up pointers is a mistake of the test: refused here."""
    rec, lib = CALLS[symbol], L.lib()
    pointers = [n for n in rec.names if ARG_TYPES[n] is L.ragged_calls._P and n != "stream"]
    null = pointers if null == "all" else null
    assert set(null) <= set(pointers), (symbol, null)
    v = dict({n: FAKE for n in pointers}, packed_cap=1 << 20, packed_readable=1 << 20, total=0, stream=None)
    v.update(values, **{n: None for n in null})
    need = rec.sizing(lib, **v)
    launches = (need and 0 < v["nchunks"] <= grid_limit(rec, v["max_chunk_bytes"]) and v["temp_bytes"] >= need
                and not set(null) & set(rec.required_pointers))
    assert not launches, f"{symbol}: these arguments pass every check"
    return rec(lib, **v)
