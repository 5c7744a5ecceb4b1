"""Which branches of the zstd frame format the zstd tests reach, asserted (tests/zstd_census.py walks the frames):
the walker itself on every frame at hand, the named edge inputs (tests/zstd_edge_inputs.py) held to the classes
and packed sizes they declare -- restatement against reference build byte for byte where that is present --, the
repeat-mode fixture (tests/golden/make_zstd_repeat.py), the hand-built frames (tests/zstd_hand_frames.py), and the
two REQUIRED sets: from here on they are the statement of what the zstd tests reach.  CPU only; the GPU runs
the same inputs and frames in tests/test_gpu_zstd_census.py."""
import functools
import json
import os
from collections import Counter

import numpy as np
import pytest

import oracle_lib as O
import zstd_census as Z
import zstd_edge_inputs as E
import zstd_hand_frames as H
from gpu_batches import sha
from test_gpu_zstd import _raw_block_frame, _rle_seq_frame
from test_zstd_golden import arrays, cases
from test_zstd_oracle import cgolden, corpus as ccorpus

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GEN_N = 1 << 20

# Every class of tests/zstd_census.py is in a REQUIRED set or named here with its reason.
# Compressor side (the fast strategy; tests/zstd_edge_inputs.py's docstring has the reasons): lit/rle/hdr1,
# {LL,OF,ML}/repeat and nseq/long cannot be written; the last four are asserted absent.
COMPRESSOR_REQUIRED = set(Z.ALL_CLASSES) - E.COMPRESSOR_NOT_REACHED - E.COMPRESSOR_UNREACHABLE
# Decoder side: every class.  (nseq/long comes from _rle_seq_frame(32769) of tests/test_gpu_zstd.py alone, a frame
# whose headers are valid and whose second sequence the reference rejects: the 3-byte count is parsed, no valid
# frame of 128 KiB blocks the decoders are given needs it.)
DECODER_REQUIRED = set(Z.ALL_CLASSES)


# ---- the fixtures and inputs, each compressed once --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_data(name):
    d = next(e for e in E.EDGES if e.name == name).make()
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def edge_packed(name, level):
    """(packed, csizes) of an edge input at one of its levels: the restatement's"""
    e = next(e for e in E.EDGES if e.name == name)
    return O.compress_chunks(edge_data(name), "zstd", e.chunk, level, use_ref=False)


EDGE_ROWS = [(e.name, lv) for e in E.EDGES for lv in e.levels]


def repeat_cases():
    with open(os.path.join(GOLD, "zstd_repeat.json")) as f:
        return json.load(f)["cases"]


@functools.lru_cache(maxsize=None)
def repeat_arrays():
    with np.load(os.path.join(GOLD, "zstd_repeat.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def repeat_corpus(c):
    if c["corpus"] == "runs":
        rng = np.random.default_rng(c["seed"])
        d = np.repeat(rng.integers(0, 4, GEN_N // 8 + 16, dtype=np.uint8), rng.integers(1, 300, GEN_N // 8 + 16))[:GEN_N]
    else:
        import lzbench_amd as L
        d = L.datagen(c["corpus"], GEN_N, c["seed"])
    return np.ascontiguousarray(d[c["offset"]: c["offset"] + c["n"]])


@functools.lru_cache(maxsize=None)
def cgolden_census():
    u = Counter()
    for c in cgolden():
        data = ccorpus(c["corpus"], c["n"], c["seed"])
        packed, cs = O.compress_chunks(data, "zstd", c["chunk"], c["level"], use_ref=False)
        u.update(Z.census_packed(packed, cs, len(data), c["chunk"])[0])     # (raises unless every walk ends exactly)
    return u


def golden_census():
    u, A = Counter(), arrays()
    for c in cases():
        u.update(Z.census_packed(A[c["name"] + "/packed"], A[c["name"] + "/csizes"], c["n"], c["chunk"])[0])
    return u


def ref_decode(frame: bytes, n: int):
    src = np.frombuffer(frame, np.uint8).copy()
    dst = np.zeros(n + 64, np.uint8)
    r = O.ref().ref_zstd_decompress(src.ctypes.data, len(frame), dst.ctypes.data, n)
    return int(r), dst[:n].tobytes()


# ---- 1. the walker ------------------------------------------------------------------------------------------------
def test_walker_ends_on_every_golden_frame():
    u = golden_census()
    assert u["block/cmp"] and u["block/raw"] and u["blocks/1"] + u["blocks/2+"] >= len(cases())


def test_walker_ends_on_every_cgolden_frame():
    u = cgolden_census()
    assert u["blocks/1"] + u["blocks/2+"] >= 195 and u["block/rle"] == 1      # (the RLE block: the 300000-zeros case)


def test_walker_counts_on_hand_built_frames():
    data = bytes(range(256)) * 16
    c, blocks, fcs = Z.walk(_raw_block_frame(data[:4000], 1000))
    assert c == Counter({"block/raw": 4, "blocks/2+": 1}) and blocks == [] and fcs == 4000
    c, blocks, fcs = Z.walk(_rle_seq_frame(1))
    assert c == Counter({"block/cmp": 1, "blocks/1": 1, "lit/raw/hdr1": 1, "nseq/1-127": 1, "LL/rle": 1, "OF/rle": 1,
                         "ML/rle": 1})
    assert blocks == [(1, 1)] and fcs == 131072
    assert Z.long_match_frames([(fcs, blocks)])          # its match is 131071 bytes
    c, blocks, _ = Z.walk(_rle_seq_frame(200))
    assert c["nseq/128-32511"] == 1 and c["lit/raw/hdr3"] == 1 and blocks == [(200, 200)]
    c, blocks, _ = Z.walk(_rle_seq_frame(32769))
    assert c["nseq/long"] == 1 and c["lit/raw/hdr3"] == 1 and blocks == [(32769, 32769)]


def test_walker_raises_off_the_last_byte():
    f = _rle_seq_frame(1)
    for bad in (f[:-1], f + b"\x00", f[:9] + f[10:], b"\x00" + f[1:], f[:4] + bytes([f[4] | 4]) + f[5:]):
        with pytest.raises(Z.CensusError):
            Z.walk(bad)
    Z.walk(f[:4] + bytes([f[4] | 4]) + f[5:] + b"\x00" * 4)       # checksum flag set: 4 more bytes belong to it


# ---- 2. the edge inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", EDGE_ROWS, ids=[f"{n}-l{lv}" for n, lv in EDGE_ROWS])
def test_edge_input_reaches_its_classes(name, level):
    e = next(e for e in E.EDGES if e.name == name)
    data = edge_data(name)
    packed, cs = edge_packed(name, level)
    if O.have_ref():
        rp, rcs = O.compress_chunks(data, "zstd", e.chunk, level, use_ref=True)
        assert (rcs == cs).all() and rp.tobytes() == packed.tobytes(), "restatement and reference build differ"
    assert len(packed) == e.packed[level]
    c, per = Z.census_packed(packed, cs, len(data), e.chunk)
    want = dict(e.classes, **e.classes_at.get(level, {}))
    short = {k: (c[k], v) for k, v in want.items() if c[k] < v}
    assert not short, f"classes lost (have, want): {short}; census {dict(c)}"
    wrong = {k: (c[k], v) for k, v in e.exact.items() if c[k] != v}
    assert not wrong, f"counts (have, want): {wrong}"
    assert e.shape is None or e.shape(per), per
    assert not any(c[k] for k in E.COMPRESSOR_UNREACHABLE), dict(c)


# ---- 3. the repeat-mode fixture -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", repeat_cases(), ids=lambda c: c["name"])
def test_repeat_fixture(case):
    A = repeat_arrays()
    data = repeat_corpus(case)
    assert sha(data) == case["input_sha256"]
    packed, cs = A[case["name"] + "/packed"], A[case["name"] + "/csizes"]
    c, _ = Z.census_packed(packed, cs, case["n"], case["chunk"])
    assert all(c[k] for k in case["classes"]), dict(c)
    if O.have_ref():
        r, out = O.decompress_chunks(packed, cs, case["n"], "zstd", case["chunk"])
        assert r == case["n"] and (out == data).all()
        rp, rcs = O.compress_chunks(data, "zstd", case["chunk"], case["level"], use_ref=True)
        assert (rcs == cs).all() and rp.tobytes() == packed.tobytes()      # (the fixture regenerates)


def test_repeat_fixture_holds_all_three_modes():
    u, A = Counter(), repeat_arrays()
    for c in repeat_cases():
        u.update(Z.census_packed(A[c["name"] + "/packed"], A[c["name"] + "/csizes"], c["n"], c["chunk"])[0])
    assert u["LL/repeat"] and u["OF/repeat"] and u["ML/repeat"]
    assert os.path.getsize(os.path.join(GOLD, "zstd_repeat.npz")) < 65536


# ---- 4. the hand-built frames -------------------------------------------------------------------------------------
HAND_CLASSES = {"rle_block": {"block/rle": 2, "block/raw": 2}, "rle_block_two": {"block/rle": 1, "block/raw": 1},
                "rle_literals_hdr1": {"lit/rle/hdr1": 1},
                "rle_literals_hdr2": {"lit/rle/hdr2": 1}, "rle_literals_hdr3": {"lit/rle/hdr3": 1},
                "no_literals": {"lit/regen=0": 1, "lit/raw/hdr1": 1}}


@pytest.mark.parametrize("name,frame,content", H.hand_frames(), ids=[h[0] for h in H.hand_frames()])
def test_hand_built_frame(name, frame, content):
    c, blocks, fcs = Z.walk(frame)
    assert fcs == len(content)
    assert all(c[k] == v for k, v in HAND_CLASSES[name].items()), dict(c)
    if not name.startswith("rle_block"):
        assert c["LL/rle"] == c["OF/rle"] == c["ML/rle"] == 1 and c["block/raw"] == 1 and len(blocks) == 1
    if O.have_ref():                     # (a frame the reference rejects is a wrong frame)
        r, out = ref_decode(frame, len(content))
        assert r == len(content), f"the reference rejects {name}"
        assert out == content


# ---- 5. what the zstd tests reach ---------------------------------------------------------------------------------
def edge_census():
    u = Counter()
    for e in E.EDGES:
        for lv in e.levels:
            u.update(Z.census_packed(*edge_packed(e.name, lv), len(edge_data(e.name)), e.chunk)[0])
    return u


def test_required_compressor_classes():
    """The frames the compressor tests hold the GPU to (the zstd_cgolden digests and the edge inputs) contain
    every class the fast strategy can write."""
    u = cgolden_census() + edge_census()
    assert not COMPRESSOR_REQUIRED - set(k for k in u if u[k]), sorted(COMPRESSOR_REQUIRED - set(u))
    assert not any(u[k] for k in E.COMPRESSOR_UNREACHABLE), {k: u[k] for k in E.COMPRESSOR_UNREACHABLE}
    assert not u["lit/rle/hdr1"]
    assert COMPRESSOR_REQUIRED | E.COMPRESSOR_NOT_REACHED | E.COMPRESSOR_UNREACHABLE == set(Z.ALL_CLASSES)


def decoder_census():
    u = golden_census() + edge_census()
    A = repeat_arrays()
    for c in repeat_cases():
        u.update(Z.census_packed(A[c["name"] + "/packed"], A[c["name"] + "/csizes"], c["n"], c["chunk"])[0])
    for _, frame, _ in H.hand_frames():
        u.update(Z.census(frame))
    for f in (_rle_seq_frame(1), _rle_seq_frame(32769), _raw_block_frame(bytes(4000), 1000)):
        u.update(Z.census(f))
    return u


def test_required_decoder_classes():
    """The frames the decoder tests run on every path -- the golden frames, the repeat-mode fixture, the hand-built
    frames and the edge inputs' frames (tests/test_gpu_zstd.py, tests/test_gpu_zstd_census.py) -- contain every
    class of the format's headers."""
    u = decoder_census()
    assert not DECODER_REQUIRED - set(k for k in u if u[k]), sorted(DECODER_REQUIRED - set(u))
    # without the edge inputs' frames: the classes only the compressor-made frames bring to the decoders
    v = u - edge_census()
    assert {k for k in DECODER_REQUIRED if not v[k]} <= {"LL/predef", "OF/predef", "nseq/0", "lit/treeless/sf0",
                                                         "lit/treeless/sf1"}
