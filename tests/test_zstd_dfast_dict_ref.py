"""CPU: the host side of the zstd level-3 dictionary call (include/lzbench_hip.h 3h) against the reference build's own
ZSTD_getParams and ZSTD_compress_usingDict (tests/zstd_dict_ref.py): the parameter function, the class bound and the
host walk of the double-fast extDict parse (lzbench_amd/csrc/zstd_dfast_dict_parse.h, the text the GPU kernel
compiles), with the branches each constructed pair reaches read off the walk's event counters."""
import ctypes as C

import numpy as np
import pytest

import lzbench_amd as L
import zstd_dfast_dict_inputs as K
import zstd_dict_inputs as I
import zstd_dict_ref as R
from test_zstd_dict_ref import replay

LEVEL = K.LEVEL


def test_params_equal_the_reference():
    R.need()
    lib = L.lib()
    for D in (8, 9, 4095, 4096, 65536, 112640, 131072):
        for n in sorted({1, 7, 64, 1000, 131072} | set(I.boundary_sizes(D))):
            out = (C.c_uint32 * 5)()
            assert lib.lzh_debug_zstd_dfast_dict_params(LEVEL, n, D, out) == 0
            c = R.lib().ZSTD_getParams(LEVEL, n, D).cParams
            assert c.strategy == 2, "not ZSTD_dfast"
            assert tuple(out[:4]) == (c.windowLog, c.hashLog, c.chainLog, c.minMatch), (D, n)
            assert out[4] == min(1 << c.windowLog, 131072)


def walk(d, c):
    """((ll, ml, offBase) rows, the event counters) of the host walk"""
    dd = np.concatenate([d, np.zeros(16, np.uint8)])
    cc = np.concatenate([c, np.zeros(16, np.uint8)])
    cap = len(c) // 4 + 16
    s = np.zeros(3 * cap, np.uint32)
    ev = np.zeros(K.NEVENTS, np.uint64)
    k = L.lib().lzh_debug_zstd_dfast_dict_parse(LEVEL, dd.ctypes.data, len(d), cc.ctypes.data, len(c), s.ctypes.data,
                                                cap, ev.ctypes.data)
    assert 0 <= k <= cap
    # the counters are optional: the same sequences without them
    s2 = np.zeros(3 * cap, np.uint32)
    assert L.lib().lzh_debug_zstd_dfast_dict_parse(LEVEL, dd.ctypes.data, len(d), cc.ctypes.data, len(c),
                                                   s2.ctypes.data, cap, None) == k and (s == s2).all()
    return s[: 3 * k].reshape(-1, 3).astype(np.int64), ev.astype(np.int64)


def check(d, c):
    seqs, ev = walk(d, c)
    assert replay(d, c, seqs) == c.tobytes()
    fields = R.block_fields(R.compress(d, c, LEVEL)) if len(c) else None
    if fields is not None:                           # (a raw block has no fields to compare)
        nseq, regen = fields
        assert len(seqs) == nseq and len(c) - int(seqs[:, 1].sum()) == regen, (len(d), len(c))
    return seqs, ev


@pytest.mark.parametrize("name,kind,d", I.dictionaries(), ids=[n for n, _, _ in I.dictionaries()])
def test_host_walk_over_the_gpu_matrix(name, kind, d):
    R.need()
    compressed = 0
    for _, c in I.chunks(kind, len(d)):
        compressed += len(check(d, c)[0]) > 0
    assert compressed > 0


@pytest.mark.parametrize("name", list(K.constructed()))
def test_constructed_pairs_reach_their_branches(name):
    R.need()
    d, c, event, expect = K.constructed()[name]
    seqs, ev = check(d, c)
    assert ev[event] > 0, f"{name}: event {K.EVENT_NAMES[event]} not reached; counters {dict(zip(K.EVENT_NAMES, ev))}"
    if expect is not None:
        at, row = expect
        assert tuple(seqs[at]) == row, f"{name}: sequence {at} is {tuple(seqs[at])}"


def test_constructed_pairs_cover_every_event():
    assert {v[2] for v in K.constructed().values()} == set(range(K.NEVENTS))


def test_the_named_pairs():
    R.need()
    P = K.pairs()
    d, c = P["largest-offset"]
    seqs, ev = check(d, c)
    assert seqs[-1][2] - 3 == len(d) + len(c) - 20 == 262124, "chunk end to dictionary start"
    seqs, ev = check(*P["cross"])
    assert ev[K.CROSSED] and ev[K.LONG_DICT], "a match from the dictionary's last bytes into the chunk's start"
    d, c = P["equal-4096"]
    seqs, ev = check(d, c)
    assert int(seqs[:, 1].sum()) > len(c) - 64, "a chunk equal to the dictionary is nearly all matches"
    seqs, ev = check(*P["dict-8"])
    assert ev[[K.REP_DICT, K.LONG_DICT, K.SHORT_DICT, K.LONG1_DICT, K.REP2_DICT]].sum() == 0, \
        "the 8-byte dictionary is not indexed: no match starts in it"


def test_class_bound():
    """the constant that sizes the table region covers the classes of every batch"""
    lib = L.lib()
    region = None
    for D in I.DICT_SIZES:
        for maxb in I.CHUNK_SIZES:
            seen = set()
            for n in sorted({1, max(maxb, 1)} | {t - D for t in [1 << s for s in range(6, 19)] + [(1 << s) + 1 for s in range(6, 19)]
                                                 if 1 <= t - D <= max(maxb, 1)}):
                out = (C.c_uint32 * 5)()
                assert lib.lzh_debug_zstd_dfast_dict_params(LEVEL, n, D, out) == 0
                seen.add((out[1], out[2], out[3]))
            need = sum((4 << h) + (4 << c) for h, c, _ in seen)
            # the region is the last of the temp layout: total(k = 0) is stage gap + scratch gap + region + gap
            region = lib.lzh_zstd_dfast_dict_compress_temp_bytes(LEVEL, D, maxb, 0) - 3 * 256
            assert len(seen) <= 11 and need <= region, (D, maxb, need, region)
    assert region == 1309952 + (-1309952) % 256
