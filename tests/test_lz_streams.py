"""CPU: the hand-built and generated LZ4 / snappy streams of tests/lz_streams.py against the restatement decoders
(oracle/lz4_oracle.c, snappy_oracle.c, frame_oracle.c) and, where oracle/_ref is built, the reference decoders
with a zeroed destination: every verdict is the case's, every accepted stream decodes to the writer's model.  No
stream is skipped.  The census sets pin what these streams add:

REQUIRED   every class here is in the census union of CASES, the generated streams, the second blocks of the
           linked frames and the HC fixture; REASON names the case each class is there for.
ABSENT     none of these is in the census of what the restatement encoders write (text, json, binary and mixed,
           1 MiB each, chunks of 65536 and 262144; LZ4 at acceleration 1 and 17, snappy).

Documented, not asserted absent: the fast LZ4 parser does reach lz4/run3x21, the window-edge offsets, lz4/ll-run255,
lz4/match-after-bulk-lit, lz4/off=pos and the limits cap-12, cap-5, cs-8 and cs-15 on these corpora (by chance of
the data: a handful of sequences each); it reaches no lz4/ml-run255, no lz4/match>window and no lz4/limit/cs-4
there, which is a property of the corpora (no long repeats), not of the parser.  The HC fixture (16 KiB of text and
binary at levels 4, 9 and 12) holds no run of 21 three-byte sequences either; lz4/run3x21 comes from the named
cases run3x40 and run3x21-lengths."""
import hashlib
import json
import os
from collections import Counter

import numpy as np
import pytest

import lz_census as Z
import lz_streams as S
import oracle_lib as O
import lzbench_amd as L

HERE = os.path.dirname(os.path.abspath(__file__))

# the case that is the reason a class is required ("random": only the generator's mix is asked for)
REASON = {
    "lz4": dict(
        [(c, f"edge-group@{c.split('@')[1]}") for c in Z.LZ4_CLASSES if "/off/" in c]
        + [(f"lz4/match>window@{kw}", f"long-match@{kw}") for kw in Z.WINDOWS]
        + [(f"lz4/overlap>window@{kw}", f"long-overlap-match@{kw}") for kw in Z.WINDOWS]
        + [("lz4/run3x21", "run3x40"), ("lz4/ll-run255", "edge-checked@4096"), ("lz4/ml-run255", "edge-checked@4096"),
           ("lz4/match-after-bulk-lit", "match-after-bulk-lit"), ("lz4/short-of-cap", "short-of-cap"),
           ("lz4/prefix-overlap", "linked-0"), ("lz4/limit/cap-12", "limit-cap-12"), ("lz4/limit/cs-8", "limit-cs-8"),
           ("lz4/limit/cap-5", "limit-cap-5"), ("lz4/limit/cs-15", "limit-cs-15"), ("lz4/limit/cs-4", "limit-cs-4"),
           ("lz4/off=pos", "offset-is-position")]),
    "snappy": dict(
        [(c, f"edge-copies@{c.split('@')[1]}") for c in Z.SNAPPY_CLASSES if "/off/" in c]
        + [("snappy/copy1", "run2-alternating"), ("snappy/copy2", "copy2-len1"), ("snappy/copy4", "copy4-69999"),
           ("snappy/lit/len0", "run2-alternating"), ("snappy/lit/len1", "lit-noncanonical"),
           ("snappy/lit/len2", "lit-noncanonical"), ("snappy/lit/len3", "lit3-66000"), ("snappy/lit/len4", "lit4-70000"),
           ("snappy/copy2/short", "copy2-len1"), ("snappy/copy/len1", "copy2-len1"),
           ("snappy/lit/noncanonical", "lit-noncanonical"), ("snappy/lit/consecutive", "lit-noncanonical"),
           ("snappy/run2x32", "run2-alternating"), ("snappy/off>65535", "copy4-69999"),
           ("snappy/copy/cross-fragment", "cross-at-start-off1"), ("snappy/tag-at-fragment", "clean-split-noncanonical"),
           ("snappy/match-after-bulk-lit", "copy-after-bulk-lit"), ("snappy/short-of-cap", "short-of-cap-tiny"),
           ("snappy/off=pos", "offset-is-position")]),
}
REQUIRED = {codec: set(REASON[codec]) for codec in REASON}
ABSENT = {
    "snappy": {"snappy/copy4", "snappy/lit/len3", "snappy/lit/len4", "snappy/copy2/short", "snappy/copy/len1",
               "snappy/lit/noncanonical", "snappy/lit/consecutive", "snappy/off>65535"},
    # an encoder fills its chunk, and a block on its own has no prefix
    "lz4": {"lz4/short-of-cap", "lz4/prefix-overlap"},
}


def _arr(b: bytes):
    return np.frombuffer(b, np.uint8).copy() if b else np.zeros(1, np.uint8)


def restatement(codec, stream, cap):
    """(size or a negative verdict, bytes) from the restatement decoder with capacity cap"""
    src, dst = _arr(stream), np.zeros(cap + 64, np.uint8)
    R = O.oracle()
    if codec == "lz4":
        r = R.oracle_lz4_decompress_safe(src.ctypes.data, len(stream), dst.ctypes.data, cap)
    else:
        r = R.oracle_snappy_uncompress(src.ctypes.data, len(stream), dst.ctypes.data, cap)
    return int(r), dst[:max(int(r), 0)].tobytes()


def snappy_length(s: bytes):
    v = sh = 0
    for c in s[:5]:
        v |= (c & 0x7F) << sh
        if c < 128:
            return v
        sh += 7
    return None


def reference(codec, stream, cap):
    """the same from the reference decoder (zeroed destination; snappy::RawUncompress has no capacity argument: a
    length above cap is refused before the call, as the chunk loop's caller would)"""
    src, dst = _arr(stream), np.zeros(cap + 64, np.uint8)
    R = O.ref()
    if codec == "lz4":
        r = R.ref_lz4_decompress_safe(src.ctypes.data, dst.ctypes.data, len(stream), cap)
        return int(r), dst[:max(int(r), 0)].tobytes()
    ulen = snappy_length(stream)
    if ulen is None or ulen > cap:
        return -1, b""
    ok = R.ref_snappy_uncompress(src.ctypes.data, len(stream), dst.ctypes.data)
    return (ulen, dst[:ulen].tobytes()) if ok else (-1, b"")


def _check(decode, codec, name, stream, cap, out, ok):
    r, got = decode(codec, stream, cap)
    assert (r >= 0) == ok, f"{codec} {name}: verdict {r}, expected {'ok' if ok else 'rejected'}"
    if ok:
        assert r == len(out), f"{codec} {name}: size {r}, model {len(out)}"
        assert got == out, f"{codec} {name}: bytes differ from the model"


def _decoders():
    return [restatement] + ([reference] if O.have_ref() else [])


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_named_cases(codec):
    cases = [c for c in S.CASES if c.codec == codec]
    assert len(cases) >= 30 and len({c.name for c in cases}) == len(cases)
    assert {256, 65536, 131072} <= {c.cap for c in cases} and max(c.cap for c in cases) <= 262144
    for decode in _decoders():
        for c in cases:
            _check(decode, codec, c.name, c.stream, c.cap, c.out, c.ok)
    for c in cases:                    # the walker gives the same verdict and size
        if c.ok:
            assert (Z.lz4 if codec == "lz4" else Z.snappy)(c.stream, c.cap)[1] == len(c.out), c.name
        else:
            with pytest.raises(Z.CensusError):
                Z.census(codec, c.stream, c.cap)


def test_limit_pairs():
    """a rule with a limit has the stream on it (accepted) and the one just past it (rejected)"""
    names = {c.name: c for c in S.CASES}
    pairs = [n for n in names if n + "-past" in names]
    assert len(pairs) >= 7
    for n in pairs:
        assert names[n].ok and not names[n + "-past"].ok, n
    for n in ("offset-is-position", "ends-on-length"):
        assert any(c.name == n and c.ok for c in S.CASES)
    for n in ("offset-past-position", "copy-past-length", "stops-before-length"):
        assert any(c.name == n and not c.ok for c in S.CASES)


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_random_streams(codec):
    sets = [(cap, lst) for cd, cap, lst in S.random_streams() if cd == codec]
    assert [(cap, len(lst)) for cap, lst in sets] == [(65536, 256), (131072, 64)]
    for decode in _decoders():
        for cap, lst in sets:
            for i, (stream, out) in enumerate(lst):
                _check(decode, codec, f"random-{cap}-{i}", stream, cap, out, True)


def frame_verdict(f, use_ref=False):
    """(size or negative, bytes) of a frame from the restatement (or the reference LZ4F_decompress)"""
    src, dst = _arr(f.frame), np.zeros(f.part + 64, np.uint8)
    if use_ref:
        r = O.ref().ref_lz4f_decompress(src.ctypes.data, len(f.frame), dst.ctypes.data, f.part)
    else:
        fn = O.oracle().oracle_lz4f_decompress if f.codec == "lz4f" else O.oracle().oracle_nvlz4_decompress
        r = fn(src.ctypes.data, len(f.frame), dst.ctypes.data, f.part)
    return int(r), dst[:max(int(r), 0)].tobytes()


def test_frames():
    frames = S.frames()
    kinds = Counter((f.codec, f.name.split("-")[0], f.out is not None) for f in frames)
    for k in (("lz4f", "independent"), ("lz4f", "linked"), ("nvlz4", "container")):
        assert kinds[k + (True,)] >= 8 and kinds[k + (False,)] >= 1, kinds
    for f in frames:
        assert len(f.frame) != f.part
        for use_ref in [False] + ([True] if O.have_ref() and f.codec == "lz4f" else []):
            r, got = frame_verdict(f, use_ref)
            if f.out is None:
                assert r != f.part and r < 0, (f.name, use_ref, r)
            else:
                assert r == f.part and got == f.out, (f.name, use_ref, r)


def linked_block_census():
    """the census of the second block of every accepted linked frame (decoded after 64 KiB of prefix)"""
    u = Counter()
    for f in S.frames():
        if f.name.startswith("linked") and f.out is not None:
            n0 = int.from_bytes(f.frame[7:11], "little")
            at = 11 + n0
            n1 = int.from_bytes(f.frame[at:at + 4], "little")
            c, n = Z.lz4(f.frame[at + 4: at + 4 + n1], S.BLOCK, prefix=S.BLOCK)
            assert n == S.BLOCK
            u.update(c)
    return u


def hc_fixture():
    """[(meta, stream, input)] of tests/golden/lz4hc.*"""
    meta = json.load(open(os.path.join(HERE, "golden", "lz4hc.json")))
    A = np.load(os.path.join(HERE, "golden", "lz4hc.npz"))
    return [(m, A[m["name"]].tobytes(), L.datagen(m["corpus"], m["n"], seed=m["seed"])) for m in meta]


def test_hc_fixture():
    fx = hc_fixture()
    assert {(m["corpus"], m["level"]) for m, _, _ in fx} == {(c, lv) for c in ("text", "binary") for lv in (4, 9, 12)}
    assert os.path.getsize(os.path.join(HERE, "golden", "lz4hc.npz")) < 65536
    for m, stream, data in fx:
        assert hashlib.sha256(data.tobytes()).hexdigest() == m["input_sha256"]
        assert len(stream) == m["stream_bytes"] and hashlib.sha256(stream).hexdigest() == m["stream_sha256"]
        for decode in _decoders():
            _check(decode, "lz4", m["name"], stream, m["n"], data.tobytes(), True)
        if O.have_ref_hc():    # the reference HC parser still writes these bytes
            out = np.zeros(m["n"] + 256, np.uint8)
            r = O.ref().ref_lz4_compress_hc(data.ctypes.data, out.ctypes.data, m["n"], len(out), m["level"])
            assert out[:r].tobytes() == stream, m["name"]


def union_census():
    u = {"lz4": Counter(), "snappy": Counter()}
    for c in S.CASES:
        if c.ok:
            u[c.codec].update(Z.census(c.codec, c.stream, c.cap))
    for codec, cap, lst in S.random_streams():
        for stream, _ in lst:
            u[codec].update(Z.census(codec, stream, cap))
    u["lz4"].update(linked_block_census())
    for m, stream, _ in hc_fixture():
        u["lz4"].update(Z.lz4(stream, m["n"])[0])
    return u


def test_required_classes():
    u = union_census()
    names = {(c.codec, c.name): c for c in S.CASES}
    for codec in ("lz4", "snappy"):
        assert REQUIRED[codec] >= set(Z.LZ4_CLASSES if codec == "lz4" else Z.SNAPPY_CLASSES)
        missing = sorted(k for k in REQUIRED[codec] if not u[codec][k])
        assert not missing, missing
        for cls, name in REASON[codec].items():        # the named case holds the class it is named for
            if name.startswith("linked"):
                assert linked_block_census()[cls]
                continue
            c = names[(codec, name)]
            assert c.ok and Z.census(codec, c.stream, c.cap)[cls], (cls, name)


def encoder_census():
    u = {"lz4": Counter(), "snappy": Counter()}
    for corpus in ("text", "json", "binary", "mixed"):
        data = L.datagen(corpus, 1 << 20, seed=5)
        for chunk in (65536, 262144):
            for codec, level in (("lz4fast", 1), ("lz4fast", 17), ("snappy", 0)):
                packed, cs = O.compress_chunks(data, codec, chunk, level)
                pos = 0
                for i, n in enumerate(cs):
                    s = packed[pos: pos + int(n)].tobytes()
                    pos += int(n)
                    part = min(chunk, len(data) - i * chunk)
                    if len(s) == part:
                        continue                       # stored raw
                    kind = "snappy" if codec == "snappy" else "lz4"
                    c, size = (Z.snappy if kind == "snappy" else Z.lz4)(s, part)
                    assert size == part
                    u[kind].update(c)
    return u


def test_absent_from_encoder_output():
    u = encoder_census()
    for codec in ("lz4", "snappy"):
        assert sum(u[codec].values()) > 0
        present = sorted(k for k in ABSENT[codec] if u[codec][k])
        assert not present, f"the {codec} encoder writes {present}"
        assert ABSENT[codec] <= REQUIRED[codec]
    print("\nLZ4 classes the fast parser reaches on these corpora:", sorted(k for k in u["lz4"] if u["lz4"][k]))


# ---- the walker itself: hand-checked streams
def test_walker_lz4_by_hand():
    # 4 literals, a 3-byte sequence (offset 1, length 4), last literals "12345": 4 + 4 + 5 = 13 bytes
    s = bytes([0x40]) + b"abcd" + bytes([1, 0]) + bytes([0x50]) + b"12345"
    c, n = Z.lz4(s, 64)
    assert n == 13 and c == Counter({"lz4/limit/cs-8": 1, "lz4/short-of-cap": 1})
    # 1 literal, offset 1 = the position, match length 15 + 255 + 1 + 4 = 275, then 5 literals
    s = bytes([0x1F]) + b"x" + bytes([1, 0, 255, 1]) + bytes([0x50]) + b"12345"
    c, n = Z.lz4(s, 281)
    assert n == 281 and c == Counter({"lz4/ml-run255": 1, "lz4/off=pos": 1, "lz4/limit/cap-5": 1})
    # literals only: the token and 15 + 1 literals
    s = bytes([0xF0, 1]) + bytes(16)
    assert Z.lz4(s, 16) == (Counter(), 16)
    for bad in (s[:-1], bytes([0x40]) + b"abcd" + bytes([5, 0]) + bytes([0x50]) + b"12345",
                bytes([0x40]) + b"abcd" + bytes([1, 0]) + bytes([0x40]) + b"1234", b""):
        with pytest.raises(Z.CensusError):
            Z.lz4(bad, 64)


def test_walker_snappy_by_hand():
    # length 11: literal "abc", COPY_1 offset 3 length 4, COPY_2 offset 7 length 1, literal "xyz" with one length byte
    s = bytes([11, 2 << 2]) + b"abc" + bytes([1, 3]) + bytes([2, 7, 0]) + bytes([60 << 2, 2]) + b"xyz"
    c, n = Z.snappy(s, 11)
    assert n == 11 and c == Counter({"snappy/lit/len0": 1, "snappy/copy1": 1, "snappy/copy2": 1, "snappy/copy2/short": 1,
                                      "snappy/copy/len1": 1, "snappy/off=pos": 2, "snappy/lit/len1": 1,
                                      "snappy/lit/noncanonical": 1})
    # two literals in a row, then a COPY_4 of 2 bytes at offset 2, into 16 bytes of room
    s = bytes([4, 0]) + b"a" + bytes([0]) + b"b" + bytes([3 | 1 << 2, 2, 0, 0, 0])
    c, n = Z.snappy(s, 16)
    assert n == 4 and c == Counter({"snappy/lit/len0": 2, "snappy/lit/consecutive": 1, "snappy/copy4": 1,
                                     "snappy/off=pos": 1, "snappy/short-of-cap": 1})
    # a 4-byte length for one byte
    s = bytes([1, 63 << 2, 0, 0, 0, 0]) + b"q"
    assert Z.snappy(s, 1) == (Counter({"snappy/lit/len4": 1, "snappy/lit/noncanonical": 1}), 1)
    for bad in (s[:-1], s[:4], bytes([2, 0]) + b"a" + bytes([1, 2]), bytes([5, 0]) + b"a"):
        with pytest.raises(Z.CensusError):
            Z.snappy(bad, 16)


def test_writers_assert_validity():
    w = S.Lz4Writer().seq(b"abcd", 5, 4).last(b"12345")          # offset past the position
    with pytest.raises(AssertionError):
        w.finish(64)
    w = S.Lz4Writer().seq(b"abcd", 1, 4).last(b"1234")           # four last literals after a match
    with pytest.raises(AssertionError):
        w.finish(64)
    w = S.Lz4Writer().seq(b"abcd", 1, 4).last(b"12345")
    with pytest.raises(AssertionError):
        w.finish(12)                                              # 13 bytes into a capacity of 12
    with pytest.raises(AssertionError):
        w.finish(len(w.s))                                        # a stream of cap bytes reads as stored raw
    assert w.finish(16) and w.expected == b"abcddddd12345"
    with pytest.raises(AssertionError):
        S.SnappyWriter().lit(b"abc").copy(4, 2, 2).finish(64)
    s = S.SnappyWriter().lit(b"abc").copy(2, 5, 2)
    assert bytes(s.out) == b"abcbcbcb" and s.finish(64) == bytes([8, 2 << 2]) + b"abc" + bytes([2 | 4 << 2, 2, 0])
