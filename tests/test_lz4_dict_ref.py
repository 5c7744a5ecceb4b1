"""CPU: the fixtures of the LZ4 dictionary tests against the reference build's own functions (tests/lz4_dict_ref.py):
the six symbols resolve, the chunks the GPU test names compress better with the dictionary, and every constructed
case produces the event it was built for -- read off the reference's output."""
import numpy as np
import pytest

import lz4_dict_inputs as I
import lz4_dict_ref as R
import lz_census
import oracle_lib as O

# the GPU cases named "compresses better with the dictionary" (tests/test_gpu_lz4_dict.py)
BETTER = [("json", 1000), ("json", 4096)]


def sequences(block: bytes):
    """[(literals, offset, match length)] of a valid LZ4 block; the last entry is (literals, 0, 0)."""
    out, ip = [], 0
    while True:
        tok = block[ip]
        ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                lit += block[ip]
                ip += 1
                if block[ip - 1] != 255:
                    break
        ip += lit
        if ip == len(block):
            out.append((lit, 0, 0))
            return out
        off = block[ip] | block[ip + 1] << 8
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                ml += block[ip]
                ip += 1
                if block[ip - 1] != 255:
                    break
        out.append((lit, off, ml + 4))


def test_the_reference_exports_the_six_functions():
    """the GPU tests skip by symbol (lz4_dict_ref.need); wherever the reference build is present they must not"""
    if not O.have_ref():
        pytest.skip("no reference build (oracle/_ref/libref.so)")
    assert R.missing() == []


def test_roundtrip_through_the_reference():
    R.need()
    d = I.dictionary("json", 4095)
    for name, c in I.chunks():
        b = R.compress(d, c)
        st, got = R.decompress(d, b, len(c))
        assert st == len(c) and got == c.tobytes(), name


@pytest.mark.parametrize("kind,size", BETTER)
def test_named_chunks_compress_better_with_the_dictionary(kind, size):
    R.need()
    c, d = I.chunk(kind, size), I.dictionary(kind, 65536)
    with_d, without = len(R.compress(d, c)), len(R.compress_plain(c))
    assert with_d < without, (with_d, without)


def test_plain_reference_is_the_oracle():
    """the comparison above is against LZ4_compress_fast, which is what lzh_compress_ragged_async writes"""
    R.need()
    c = I.chunk("json", 4096)
    assert R.compress_plain(c) == O.lz4_compress(c, 1)


def test_constructed_cases_produce_their_events():
    R.need()
    C = I.constructed()
    for name, (d, c) in C.items():
        b = R.compress(d, c)
        cnt, size = lz_census.lz4(b, len(c), prefix=len(d))      # (a valid block of the chunk's size)
        assert size == len(c), name
    d, c = C["equal-4095"]                       # a match at the dictionary's own distance over most of the chunk
    s = sequences(R.compress(d, c))
    assert any(off == len(d) and ml > len(c) // 2 for _, off, ml in s), s[:3]
    d, c = C["equal-65536"]                      # (its own distance is one past the largest offset: other matches)
    s = sequences(R.compress(d, c))
    assert len(s) > 1 and all(off <= 65535 for _, off, _ in s)
    d, c = C["tail40-cross"]
    b = R.compress(d, c)
    s = sequences(b)
    # the first sequence starts at chunk position 0 (probing starts at 1: the catch-up stepped back over the
    # boundary), 40 bytes into the dictionary, and runs past the boundary into the chunk
    assert s[0] == (0, 40, 80), s[:2]
    assert lz_census.lz4(b, len(c), prefix=len(d))[0]["lz4/prefix-overlap"] == 1
    d, c = C["slot0-65536"]
    assert sequences(R.compress(d, c)) == [(len(c), 0, 0)]       # index 0 is 65537 away: rejected, literals only
    d, c = C["dist-65535"]
    s = sequences(R.compress(d, c))              # the run, then the match into the dictionary at the largest offset
    assert s[0][:2] == (1, 1) and s[1] == (0, 65535, 10), s[:3]
    d, c = C["dist-65536"]
    s = sequences(R.compress(d, c))
    assert s[0][:2] == (1, 1) and all(off <= 1 for _, off, _ in s), s[:3]
    d, c = C["raw-store"]
    assert len(R.compress(d, c)) == len(c) and R.packed(d, c) == c.tobytes()


def test_chunks_under_13_bytes_are_literals_only():
    R.need()
    d = I.dictionary("text", 65536)
    for size in (0, 1, 12):
        c = I.chunk("text", size)
        assert sequences(R.compress(d, c)) == [(size, 0, 0)]
    assert R.compress(d, I.chunk("text", 0)) == b"\x00"
