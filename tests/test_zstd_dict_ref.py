"""CPU: the host side of the zstd dictionary calls (include/lzbench_hip.h 3f) against the reference build's own
ZSTD_getParams and ZSTD_compress_usingDict (tests/zstd_dict_ref.py): the parameter function and the host walk of the
extDict parse (lzbench_amd/csrc/zstd_dict_parse.h, the text the GPU kernel compiles)."""
import ctypes as C

import numpy as np
import pytest

import lzbench_amd as L
import zstd_dict_inputs as I
import zstd_dict_ref as R


def test_every_needed_symbol_resolves():
    """so that R.need()'s skip cannot hide a missing export where the reference build exists"""
    import oracle_lib as O
    if not O.have_ref():
        pytest.skip("no reference build")
    assert R.missing() == []


@pytest.mark.parametrize("level", [1, -1, -5])
def test_params_equal_the_reference(level):
    R.need()
    lib = L.lib()
    for D in (8, 9, 4095, 4096, 65536, 112640, 131072):
        for n in sorted({1, 7, 64, 1000, 131072} | set(I.boundary_sizes(D))):
            out = (C.c_uint32 * 5)()
            assert lib.lzh_debug_zstd_dict_params(level, n, D, out) == 0
            w, h, mm, tl, strat = R.cparams(level, n, D)
            assert strat == 1, "not ZSTD_fast"
            assert tuple(out[:4]) == (w, h, mm, tl), (level, D, n)
            assert out[4] == min(1 << w, 131072)


def walk(level, d, c):
    dd = np.concatenate([d, np.zeros(16, np.uint8)])
    cc = np.concatenate([c, np.zeros(16, np.uint8)])
    cap = len(c) // 4 + 16
    s = np.zeros(3 * cap, np.uint32)
    k = L.lib().lzh_debug_zstd_dict_parse(level, dd.ctypes.data, len(d), cc.ctypes.data, len(c), s.ctypes.data, cap)
    assert 0 <= k <= cap
    return s[: 3 * k].reshape(-1, 3).astype(np.int64)


def replay(d, c, seqs):
    """the chunk rebuilt from the sequences over dictionary and chunk (literals read from the chunk itself)"""
    out = bytearray()
    rep = [1, 4, 8]
    D = len(d)
    for ll, ml, ob in seqs:
        out += c[len(out): len(out) + ll].tobytes()
        if ob > 3:
            off = ob - 3
            rep = [off, rep[0], rep[1]]
        else:                                        # offBase 1 with literals: rep[0]; without: rep[1], swapped
            assert ob == 1
            if ll == 0:
                rep = [rep[1], rep[0], rep[2]]
            off = rep[0]
        assert off <= len(out) + D, "offset before the dictionary's first byte"
        for _ in range(ml):
            p = len(out) - off
            out.append(int(d[D + p]) if p < 0 else out[p])
    out += c[len(out):].tobytes()
    return bytes(out)


def check(level, d, c):
    seqs = walk(level, d, c)
    assert replay(d, c, seqs) == c.tobytes()
    fields = R.block_fields(R.compress(d, c, level)) if len(c) else None
    if fields is not None:                           # (a raw block has no fields to compare)
        nseq, regen = fields
        assert len(seqs) == nseq and len(c) - int(seqs[:, 1].sum()) == regen, (level, len(d), len(c))
    return seqs


@pytest.mark.parametrize("name,kind,d", I.dictionaries(), ids=[n for n, _, _ in I.dictionaries()])
def test_host_walk_over_the_gpu_matrix(name, kind, d):
    R.need()
    compressed = 0
    for _, c in I.chunks(kind, len(d)):
        for level in I.LEVELS:
            compressed += len(check(level, d, c)) > 0
    assert compressed > 0 or len(d) < 12


def test_constructed_cases_reach_their_branches():
    R.need()
    K = I.constructed()
    for name, (d, c) in K.items():
        for level in I.LEVELS:
            check(level, d, c)
    s = check(1, *K["cross"])
    assert tuple(s[0]) == (0, 80, 40 + 3), "a match from the dictionary's last 40 bytes on into the chunk's own start"
    d, c = K["catchup-dict-start"]
    assert tuple(check(1, d, c)[0]) == (6, 60, 6 + len(d) + 3), "the catch-up reaches the dictionary's first byte"
    s = check(1, *K["catchup-chunk-start"])
    assert tuple(s[0]) == (68, 60, 68 + 3), "the catch-up reaches the chunk's first byte"
    s = check(1, *K["rep-in-dict"])
    assert tuple(s[1]) == (1, 39, 1) and s[0][2] - 3 > 20 + 1, "a repcode at ip + 1 with its source in the dictionary"
    s = check(1, *K["rep-excluded"])
    assert len(s) == 1 or tuple(s[1])[2] != 1 or s[1][0] != 7, "the excluded repcode was taken"
    s = check(1, *K["offset2-in-dict"])
    assert tuple(s[2]) == (0, 20, 1), "the offset_2 loop with its source in the dictionary"
    d, c = K["largest-offset"]
    assert check(1, d, c)[-1][2] - 3 == len(d) + len(c) - 20 == 262124, "chunk end to dictionary start"


@pytest.mark.parametrize("level", [-1, -2, -4, -5])
def test_host_walk_at_the_other_levels(level):
    """the inputs of tests/test_gpu_zstd_dict.py's test_the_other_levels (targetLength is the parse's step)"""
    R.need()
    for d, c in I.constructed().values():
        check(level, d, c)
    dt = I.dictionary("text", 4095)
    assert sum(len(check(level, dt, I.chunk("text", s))) for s in (300, 4099, 16385)) > 0


def test_separate_and_adjacent_dictionary_give_other_bytes():
    """the reference runs another parser when the chunk starts where the dictionary ends: the helper must not do that"""
    R.need()
    d, c = I.dictionary("text", 4096), I.chunk("text", 5000)
    a, b = R.compress(d, c, 1), R.compress_adjacent(d, c, 1)
    assert a != b
    assert R.decompress(d, a, len(c)) == R.decompress(d, b, len(c)) == (len(c), c.tobytes())
    plain = R.compress_plain(c, 1)
    assert len(a) < len(plain)
