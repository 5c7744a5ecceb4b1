"""tests/lz_streams.py -- valid LZ4 blocks and snappy streams that the project's encoders never write, with the
bytes they must decode to.  Pure Python; the GPU tests (test_gpu_lz_streams.py) and the CPU tests
(test_lz_streams.py) share it.

SnappyWriter and Lz4Writer build a stream from explicit operations and keep, byte by byte, the output it must
decode to: that model is the expected value of every test.  finish(cap) asserts that the stream is valid for a
decoder with capacity cap (offsets inside the output, the LZ4 end-of-block rules, a size other than cap, which the
chunk loop would take for a chunk stored raw); finish(cap, valid=False) returns a stream built to be rejected.

CASES            named streams (codec, name, cap, stream, expected_out, expect_ok); a rule with a limit has a
                 pair, the stream on the limit and the one just past it
random_valid()   a seeded generator of valid streams with every tag kind and length form at equal weight
random_streams() [(codec, cap, [(stream, expected_out)])]: 256 streams per codec at 65536, 64 at 131072
frames()         LZ4 blocks of the above wrapped as LZ4 frames (independent and linked blocks) and nvcomp containers"""
from collections import namedtuple

import numpy as np

import lz_census as Z

Case = namedtuple("Case", "codec name cap stream out ok")
WINDOWS = Z.WINDOWS


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _extend_copy(out: bytearray, off: int, ln: int):
    """out[p + t] = out[p - off + t], byte by byte (an overlapping copy repeats its period)"""
    p = len(out)
    if off >= ln:
        out += out[p - off: p - off + ln]
    else:
        pat = bytes(out[p - off:])
        out += (pat * (ln // off + 1))[:ln]


class SnappyWriter:
    def __init__(self):
        self.tags = bytearray()
        self.out = bytearray()
        self.valid = True

    def lit(self, b: bytes, form=None):
        """a literal; form None: the shortest tag, 0: the length in the tag (up to 60 bytes), 1..4: that many
        length bytes"""
        n = len(b) - 1
        assert n >= 0
        if form is None:
            form = 0 if n < 60 else (n.bit_length() + 7) >> 3
        if form == 0:
            assert n < 60
            self.tags.append(n << 2)
        else:
            assert n < 1 << (8 * form)
            self.tags.append((59 + form) << 2)
            self.tags += n.to_bytes(form, "little")
        self.tags += b
        self.out += b
        return self

    def copy(self, off: int, ln: int, kind: int = 2):
        if kind == 1:
            assert 4 <= ln <= 11 and 0 <= off < 2048
            self.tags += bytes([1 | (ln - 4) << 2 | (off >> 8) << 5, off & 255])
        else:
            assert kind in (2, 4) and 1 <= ln <= 64 and 0 <= off < 1 << (8 * kind)
            self.tags += bytes([(2 if kind == 2 else 3) | (ln - 1) << 2]) + off.to_bytes(kind, "little")
        if 0 < off <= len(self.out):
            _extend_copy(self.out, off, ln)
        else:
            self.valid = False
        return self

    def raw(self, b: bytes):
        """bytes put into the tag stream as they are (rejected streams)"""
        self.tags += b
        self.valid = False
        return self

    def finish(self, cap: int, valid: bool = True, ulen=None) -> bytes:
        s = varint(len(self.out) if ulen is None else ulen) + bytes(self.tags)
        if valid:
            assert self.valid and ulen is None and len(self.out) <= cap
        assert len(s) != cap, "a stream of cap bytes reads as a chunk stored raw"
        return s


class Lz4Writer:
    def __init__(self, prefix: bytes = b""):
        self.s = bytearray()
        self.out = bytearray(prefix)
        self.prefix = len(prefix)
        self.recs = []          # per sequence: (length-byte positions, literal end in the stream, ..) for finish()
        self.closed = False
        self.valid = True

    @property
    def pos(self):
        return len(self.out) - self.prefix

    def _len(self, v):
        """the length bytes of a nibble-15 field holding v >= 15"""
        v -= 15
        return bytes([255] * (v // 255) + [v % 255])

    def seq(self, lits: bytes, off: int, mlen: int):
        assert not self.closed and mlen >= 4 and 0 <= off < 65536
        ll, ml = len(lits), mlen - 4
        tok_at = len(self.s)
        self.s.append(min(ll, 15) << 4 | min(ml, 15))
        lb = self._len(ll) if ll >= 15 else b""
        self.s += lb + lits
        lit_end, op_lit = len(self.s), self.pos + ll
        self.s += off.to_bytes(2, "little")
        mb = self._len(ml) if ml >= 15 else b""
        self.s += mb
        self.out += lits
        if 0 < off <= len(self.out):
            _extend_copy(self.out, off, mlen)
        else:
            self.valid = False
        self.recs.append((tok_at, len(lb), lit_end, op_lit, len(mb), len(self.s), op_lit + mlen))
        return self

    def last(self, lits: bytes):
        assert not self.closed
        ll = len(lits)
        tok_at = len(self.s)
        self.s.append(min(ll, 15) << 4)
        lb = self._len(ll) if ll >= 15 else b""
        self.s += lb + lits
        self.out += lits
        self.recs.append((tok_at, len(lb), len(self.s), self.pos, 0, len(self.s), None))
        self.closed = True
        return self

    def raw(self, b: bytes):
        self.s += b
        self.valid = False
        return self

    @property
    def expected(self) -> bytes:
        return bytes(self.out[self.prefix:])

    def finish(self, cap: int, valid: bool = True) -> bytes:
        s, cs = bytes(self.s), len(self.s)
        assert cs != cap, "a stream of cap bytes reads as a chunk stored raw"
        if not valid:
            return s
        assert self.valid and self.closed and self.pos <= cap
        # the end-of-block rules of LZ4_decompress_safe (lz4.c:1929-2151), from the recorded positions
        for tok_at, nlb, lit_end, op_lit, nmb, end, op_end in self.recs:
            if nlb:   # the first length byte below cs - 15, and every 255 read before that limit
                assert tok_at + 1 < cs - 15 and tok_at + nlb < cs - 15 + 1, "literal length bytes"
            if op_end is None:
                assert lit_end == cs
                continue
            assert op_lit <= cap - 12 and lit_end <= cs - 8, "a sequence on the last-literals limits"
            assert not nmb or end < cs - 4, "match length bytes"
            assert op_end <= cap - 5, "match past cap - 5"
        return s


# ---------------------------------------------------------------------------------------------- named cases
def _rb(rng, n) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _lz4_lits(w: Lz4Writer, rng, upto: int):
    """random literals (sequences of up to 200 literals and a 4-byte near match) to at least `upto` output bytes"""
    while w.pos < upto:
        lits = _rb(rng, int(rng.integers(1, 200)))
        w.seq(lits, int(rng.integers(1, min(w.pos + len(lits), 60) + 1)), 4)
    return w


def _lz4_close(w: Lz4Writer, rng, cap: int, full: bool = True) -> bytes:
    """end the block: with full, literals up to exactly cap bytes of output"""
    room = cap - w.pos
    assert room >= 5
    w.last(_rb(rng, room if full else 5))
    return w.finish(cap)


def _lz4_start(rng, upto: int) -> Lz4Writer:
    w = Lz4Writer()
    w.seq(_rb(rng, 40), 7, 9)
    return _lz4_lits(w, rng, upto)


def _lz4_cases():
    rng = np.random.default_rng(20261)
    cases = []

    def add(name, cap, w, full=True):
        cases.append(Case("lz4", name, cap, _lz4_close(w, rng, cap, full), w.expected, True))

    def exact(name, cap, w):                       # (the writer has ended the block itself)
        cases.append(Case("lz4", name, cap, w.finish(cap), w.expected, True))

    def reject(name, cap, w):
        cases.append(Case("lz4", name, cap, w.finish(cap, valid=False), b"", False))

    for kw in WINDOWS:
        edges = list(Z.EDGES(kw))
        band = list(range(kw - 131, kw + 3))
        # group members (short lengths) at the edge offsets and across the near / far band, at shifting alignments
        w = _lz4_start(rng, kw + 300)
        for rep in range(2):
            for o in edges + band:
                w.seq(_rb(rng, int(rng.integers(0, 4)) + rep), o, 4 + (o + rep) % 15)
        for o in edges:                        # more than one 128-byte pass per member
            w.seq(_rb(rng, int(rng.integers(0, 20))), o, int(rng.integers(100, 273)))
        add(f"edge-group@{kw}", 65536, w)
        # the same through the checked path: 255-run match and literal lengths
        w = _lz4_start(rng, kw + 300)
        for o in edges + band[::9]:
            w.seq(_rb(rng, int(rng.integers(0, 10))), o, int(rng.integers(274, 700)))
            w.seq(_rb(rng, int(rng.integers(270, 500))), o, int(rng.integers(4, 19)))
        add(f"edge-checked@{kw}", 65536, w, full=False)
        # matches longer than the window at those offsets (far, non-overlapping: the shape of the zstd bug)
        w = _lz4_start(rng, kw + 300)
        for o in edges + [kw - 100]:
            w.seq(_rb(rng, int(rng.integers(0, 30))), o, kw + int(rng.integers(1, 700)))
        add(f"long-match@{kw}", 131072, w)
        # ... and overlapping ones at a period shorter than a wave: the match comes round the window onto the bytes
        # it started from (SinkT::match read them there for the whole match: wrong bytes from KW on, unless the
        # period divides the window)
        w = _lz4_start(rng, 300)
        for o in (3, 62, 7, 63):
            w.seq(_rb(rng, int(rng.integers(0, 30))), o, kw + int(rng.integers(1, 700)))
        w.seq(_rb(rng, 2), 62, kw - 62).seq(_rb(rng, 2), 62, kw - 61)      # the last length that fits, the first that wraps
        add(f"long-overlap-match@{kw}", 131072, w)
        w = _lz4_start(rng, kw + 2)            # twice the window, one match to the end of the block
        w.seq(b"", kw + 1, 65536 - 5 - w.pos)
        add(f"long-match-to-the-end@{kw}", 65536, w)

    # dense chains of 3-byte sequences; the sources are bytes earlier members of the same pass produce
    w = Lz4Writer()
    w.seq(_rb(rng, 8), 3, 4)
    for i in range(40):
        w.seq(b"", 1 + i % 7, 4)
    add("run3x40", 256, w, full=False)
    w = _lz4_start(rng, 500)
    for rep in range(4):
        for i in range(21 + rep):
            w.seq(b"", int(rng.integers(1, 25)), int(rng.integers(4, 19)))
        w.seq(_rb(rng, 3 + rep), 200, 30)
    add("run3x21-lengths", 65536, w)

    # a match right after a bulk literal run (the window restarts after it)
    w = _lz4_start(rng, 700)
    for o in (1, 2, 3, 7, 31, 63):
        w.seq(_rb(rng, 513 + o), o, 4 + o % 15)            # the match as a group member
        w.seq(_rb(rng, 600), o, 300 + o)                   # ... and through the checked path
    add("match-after-bulk-lit", 65536, w)

    # the first byte as a source, and one before it
    w = Lz4Writer()
    w.seq(_rb(rng, 20), 20, 12).seq(_rb(rng, 1), 33, 40)
    add("offset-is-position", 256, w, full=False)
    w = Lz4Writer()
    w.seq(_rb(rng, 20), 21, 12).last(_rb(rng, 8))
    reject("offset-past-position", 256, w)
    w = _lz4_start(rng, 3000)
    w.seq(_rb(rng, 5), w.pos + 6, 12).last(_rb(rng, 8))
    reject("offset-past-position-late", 65536, w)

    # short of the capacity
    w = Lz4Writer()
    w.seq(_rb(rng, 30), 11, 50)
    add("short-of-cap", 65536, w, full=False)
    add("short-of-cap-literals-only", 65536, Lz4Writer(), full=False)

    # ---- the end-of-block limits, cap 256: on the limit and one past it
    cap = 256
    for past in (0, 1):
        # literals of a sequence may end at cap - 12
        w = Lz4Writer()
        w.seq(_rb(rng, cap - 12 + past), 5, 4).last(_rb(rng, 5))
        (reject if past else exact)(f"limit-cap-12{'-past' if past else ''}", cap, w)
        # ... and in the stream at cs - 8: five last literals, or four
        w = Lz4Writer()
        w.seq(_rb(rng, 60), 5, 9).last(_rb(rng, 5 - past))
        (reject if past else exact)(f"limit-cs-8{'-past' if past else ''}", cap, w)
        # a match may end at cap - 5
        w = Lz4Writer()
        w.seq(_rb(rng, 100), 50, cap - 5 - 100 + past).last(_rb(rng, 5 - past))
        (reject if past else exact)(f"limit-cap-5{'-past' if past else ''}", cap, w)
        # a match-length byte is read below cs - 4: token, four literals after it; or three
        w = Lz4Writer()
        w.seq(_rb(rng, 60), 5, 19 + 7).last(_rb(rng, 4 - past))
        (reject if past else exact)(f"limit-cs-4{'-past' if past else ''}", cap, w)
    # a literal-length byte is read below cs - 15: the last sequence with exactly 15 literals
    w = Lz4Writer()
    w.seq(_rb(rng, 30), 5, 9).last(_rb(rng, 15))
    exact("limit-cs-15", cap, w)
    w = Lz4Writer()
    w.seq(_rb(rng, 30), 5, 9).raw(b"\xf0\x00" + _rb(rng, 14))
    reject("limit-cs-15-past", cap, w)
    w = Lz4Writer()
    w.seq(_rb(rng, 30), 5, 9).raw(b"\xf0\xff" + _rb(rng, 15))      # a 255 whose successor would pass the limit
    reject("limit-cs-15-run-cut", cap, w)
    # the same limits far into a block of 65536
    w = _lz4_start(rng, 60000)
    w.seq(_rb(rng, 65536 - 12 - w.pos), 4000, 4).last(_rb(rng, 5))
    exact("limit-cap-12-late", 65536, w)
    w = _lz4_start(rng, 60000)
    w.seq(_rb(rng, 65536 - 11 - w.pos), 4000, 4).last(_rb(rng, 5))
    reject("limit-cap-12-late-past", 65536, w)
    w = _lz4_start(rng, 60000)
    w.seq(_rb(rng, 9), 4097, 65536 - 5 - 9 - w.pos).last(_rb(rng, 5))
    exact("limit-cap-5-late", 65536, w)
    w = _lz4_start(rng, 60000)
    w.seq(_rb(rng, 9), 4097, 65536 - 4 - 9 - w.pos).last(_rb(rng, 4))
    reject("limit-cap-5-late-past", 65536, w)
    return cases


def _sn_fill(s: SnappyWriter, rng, upto: int, far: bool = False):
    """random literals and short copies until exactly `upto` output bytes; copies stay inside the 64 KiB fragment
    of their first byte unless far"""
    while len(s.out) < upto:
        room = upto - len(s.out)
        pos = len(s.out)
        reach = pos if far else pos % 65536
        if reach >= 64 and room >= 8 and rng.random() < 0.5:
            s.copy(int(rng.integers(1, min(reach, 4000) + 1)), int(min(room, rng.integers(4, 65))))
        else:
            s.lit(_rb(rng, int(min(room, rng.integers(1, 300)))))
    return s


def _snappy_cases():
    rng = np.random.default_rng(20262)
    cases = []

    def add(name, cap, s, fill=None):
        if fill:
            _sn_fill(s, rng, cap, far=fill == "far")
        cases.append(Case("snappy", name, cap, s.finish(cap), bytes(s.out), True))

    def reject(name, cap, s, ulen=None):
        cases.append(Case("snappy", name, cap, s.finish(cap, valid=False, ulen=ulen), b"", False))

    # the streams of the issue's CPU check
    add("lit4-70000", 131072, SnappyWriter().lit(_rb(rng, 70000), 4))
    add("copy4-69999", 131072, SnappyWriter().lit(_rb(rng, 70000)).copy(69999, 64, 4))
    add("copy2-len1", 256, SnappyWriter().lit(_rb(rng, 9)).copy(3, 1, 2).copy(10, 1, 2).lit(b"z"))
    s = SnappyWriter().lit(_rb(rng, 5))
    for i in range(32):
        s.lit(bytes([i])).copy(1 + i % 5, 4 + i % 8, 1)
    add("run2-alternating", 65536, s)
    add("lit-noncanonical", 256, SnappyWriter().lit(_rb(rng, 7), 1).lit(_rb(rng, 60), 1).lit(_rb(rng, 3), 2)
        .lit(_rb(rng, 1), 3).lit(_rb(rng, 33), 4).lit(_rb(rng, 61), 2))

    # runs of two-byte members: 32 and 33 of them, starting at every alignment of the tag stream
    for lead in range(4):
        for n in (32, 33, 64):
            s = SnappyWriter().lit(_rb(rng, 12 + lead))
            for i in range(n):
                if (i + lead) % 2:
                    s.lit(_rb(rng, 1))
                else:
                    s.copy(int(rng.integers(1, min(len(s.out), 2047) + 1)), int(rng.integers(4, 12)), 1)
            s.lit(_rb(rng, 70))
            add(f"run2x{n}-lead{lead}", 65536, s)
    s = SnappyWriter().lit(_rb(rng, 4))
    for i in range(70):                       # COPY_1s alone, and 1-byte literals alone
        s.copy(1 + i % 4, 4 + i % 8, 1)
    for i in range(70):
        s.lit(_rb(rng, 1))
    add("run2-one-kind", 65536, s, fill="near")

    # one-byte members: every byte pair of a pass with two owners
    s = SnappyWriter().lit(_rb(rng, 16))
    for i in range(150):
        k = i % 3
        if k == 0:
            s.copy(int(rng.integers(1, 17)), 1, 2)
        elif k == 1:
            s.lit(_rb(rng, 1))
        else:
            s.copy(int(rng.integers(1, 17)), 1, 4)
    for i in range(100):
        s.copy(1 + i % 3, 1 + i % 3, 2)
    add("len1-members", 65536, s)

    # COPY_2 forms a COPY_1 could hold; COPY_4 holding small offsets; consecutive literals of every form
    s = SnappyWriter().lit(_rb(rng, 300))
    for ln in range(1, 12):
        s.copy(int(rng.integers(1, 300)), ln, 2).copy(int(rng.integers(1, 300)), ln, 4)
    for form, n in ((0, 1), (0, 60), (1, 61), (1, 256), (2, 257), (2, 4000), (3, 2), (4, 2), (3, 700), (None, 1)):
        s.lit(_rb(rng, n), form)
    add("noncanonical-mix", 65536, s, fill="near")

    # literal tags 62 and 63 inside a fragment-sized chunk, canonical and not
    add("lit3-66000", 131072, SnappyWriter().lit(_rb(rng, 66000)).copy(65999, 40, 4).lit(_rb(rng, 9), 3))
    add("lit3-lit4-small", 65536, SnappyWriter().lit(_rb(rng, 5000), 3).copy(4999, 64, 2).lit(_rb(rng, 5000), 4)
        .copy(1, 64, 2), fill="near")
    add("lit4-whole-chunk", 131072, SnappyWriter().lit(_rb(rng, 131072), 4))
    add("lit3-whole-chunk", 65536, SnappyWriter().lit(_rb(rng, 65536), 3))

    # window edges: copies at the edge offsets and across the near / far band, as group members; chains of 64-byte
    # copies at one offset stand in for matches longer than the window
    for kw in WINDOWS:
        s = _sn_fill(SnappyWriter(), rng, kw + 300)
        for rep in range(2):
            for o in list(Z.EDGES(kw)) + list(range(kw - 131, kw + 3)):
                if rep:
                    s.lit(_rb(rng, 1 + o % 3))
                s.copy(o, 1 + (o * 7 + rep) % 64, 2 if (o + rep) % 3 else 4)
        for o in Z.EDGES(kw):
            for i in range((kw + 700) // 64):
                s.copy(o, 64, 2)
            s.lit(_rb(rng, 5))
        add(f"edge-copies@{kw}", 131072, s)

    # a copy right after a bulk literal run
    s = SnappyWriter().lit(_rb(rng, 100))
    for o in (1, 2, 3, 7, 31, 63):
        s.lit(_rb(rng, 513 + o)).copy(o, 4 + o % 8, 1).lit(_rb(rng, 700), 3).copy(o, 64, 2).copy(o, 64, 4)
    add("copy-after-bulk-lit", 65536, s, fill="near")

    # two fragments: copies from fragment 1 into fragment 0, and a clean split made of non-canonical tags
    def two(name, build, fill="near"):
        s = _sn_fill(SnappyWriter(), rng, 65536)
        build(s)
        add(name, 131072, s, fill=fill)

    two("cross-at-start-off1", lambda s: s.copy(1, 64, 2))
    two("cross-at-start-off65536", lambda s: s.copy(65536, 64, 4))
    two("cross-off65535", lambda s: s.lit(_rb(rng, 100)).copy(65535, 64, 2))
    two("cross-by-one", lambda s: s.lit(_rb(rng, 64)).copy(65, 64, 2))
    two("cross-copy4-70000", lambda s: _sn_fill(s, rng, 100000).copy(70000, 64, 4))
    two("cross-late-copy1", lambda s: s.lit(_rb(rng, 5)).copy(6, 11, 1))
    two("cross-everywhere", lambda s: None, fill="far")
    s = _sn_fill(SnappyWriter(), rng, 65530)
    s.copy(100, 64, 2)                                       # a copy over the fragment start: no tag starts there
    add("copy-over-fragment-start", 131072, s, fill="near")
    s = _sn_fill(SnappyWriter(), rng, 65530)
    s.lit(_rb(rng, 6), 4).lit(_rb(rng, 3), 3).copy(2, 1, 4).lit(_rb(rng, 900), 3)
    add("clean-split-noncanonical", 131072, s, fill="near")
    two("clean-split-copy-near-start", lambda s: s.lit(_rb(rng, 1)).copy(1, 64, 4))
    for i in range(6):                        # the generator's mix of forms, written a fragment at a time
        stream, out = random_valid("snappy", rng, 131072, fragment_local=True)
        cases.append(Case("snappy", f"clean-split-mix-{i}", 131072, stream, out, True))
    s = _sn_fill(SnappyWriter(), rng, 65536)
    add("short-of-cap-one-fragment", 131072, s)
    add("short-of-cap-tiny", 65536, SnappyWriter().lit(b"abcdefgh").copy(8, 8, 2))

    # ---- limits: on and one past
    add("offset-is-position", 256, SnappyWriter().lit(_rb(rng, 20)).copy(20, 30, 2).copy(50, 5, 1).copy(55, 64, 4))
    reject("offset-past-position", 256, SnappyWriter().lit(_rb(rng, 20)).copy(21, 30, 2))
    reject("offset-past-position-copy1", 256, SnappyWriter().lit(_rb(rng, 20)).copy(21, 5, 1))
    reject("offset-past-position-copy4", 65536, _sn_fill(SnappyWriter(), rng, 5000).copy(5001, 5, 4))
    reject("offset-zero", 256, SnappyWriter().lit(_rb(rng, 20)).copy(0, 5, 2))
    reject("copy4-offset-2^31", 65536, _sn_fill(SnappyWriter(), rng, 5000).copy(1 << 31, 5, 4))
    add("ends-on-length", 256, SnappyWriter().lit(_rb(rng, 192)).copy(100, 64, 2))
    s = SnappyWriter().lit(_rb(rng, 192)).copy(100, 64, 2)
    reject("copy-past-length", 256, s, ulen=255)
    s = SnappyWriter().lit(_rb(rng, 192)).copy(100, 63, 2)
    reject("stops-before-length", 256, s, ulen=256)
    reject("length-above-capacity", 256, SnappyWriter().lit(_rb(rng, 200)).lit(_rb(rng, 57)))
    reject("literal-past-the-end", 256, SnappyWriter().lit(_rb(rng, 20)).raw(bytes([61 << 2, 0x10, 0x27]) + _rb(rng, 50)),
           ulen=120)
    reject("lit4-length-past-the-end", 65536, SnappyWriter().lit(_rb(rng, 20)).raw(bytes([63 << 2, 9, 0, 0])), ulen=30)
    reject("copy4-tag-cut", 256, SnappyWriter().lit(_rb(rng, 20)).raw(bytes([3 | 4 << 2, 5, 0, 0])), ulen=25)
    return cases


# ---------------------------------------------------------------------------------------------- the generator
def _log_uniform(rng, lo: int, hi: int) -> int:
    """an integer in [lo, hi], uniform in its logarithm"""
    if hi <= lo:
        return lo
    return int(min(hi, max(lo, round(float(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))) - 0.5)))))


def _draw_offset(rng, pos: int, limit: int) -> int:
    top = min(pos, limit)
    if rng.random() < 0.25:
        edge = [o for kw in WINDOWS for o in list(Z.EDGES(kw)) + [kw - 64, kw - 1] if o <= top]
        if edge:
            return int(edge[int(rng.integers(0, len(edge)))])
    return _log_uniform(rng, 1, top)


def random_valid(codec: str, rng, cap: int, fragment_local: bool = False):
    """(stream, expected output) of a valid stream drawn from a mix no encoder here writes: every tag kind and
    length form with equal weight, offsets log-uniform up to the position, a quarter of them window edges.
    fragment_local (snappy): the same mix, but no tag crosses a multiple of 64 KiB of output and no copy reads
    before the one its first byte is in, as in a stream written a fragment at a time"""
    short = not fragment_local and rng.random() < 0.125   # some decode to fewer bytes than the capacity
    target = int(rng.integers(1, cap)) if short else cap
    if codec == "snappy":
        s = SnappyWriter()
        s.lit(_rb(rng, int(rng.integers(1, 20))))
        while len(s.out) < target:
            room = target - len(s.out)
            op = int(rng.integers(0, 8))
            reach = len(s.out)
            if fragment_local:
                room, reach = min(room, 65536 - reach % 65536), reach % 65536
                op = op if reach else op % 5
            if op < 5:                                  # literal forms 0..4
                hi = (60, 256, 4096, 4096, 4096)[op]
                s.lit(_rb(rng, _log_uniform(rng, 1, min(hi, room))), op)
            else:
                kind = (1, 2, 4)[op - 5]
                if kind == 1:
                    if room < 4:
                        continue
                    s.copy(_draw_offset(rng, reach, 2047), int(rng.integers(4, min(11, room) + 1)), 1)
                else:
                    s.copy(_draw_offset(rng, reach, 65535 if kind == 2 else cap),
                           int(rng.integers(1, min(64, room) + 1)), kind)
        return s.finish(cap), bytes(s.out)
    w = Lz4Writer()
    w.seq(_rb(rng, int(rng.integers(1, 20))), 1, 4)
    while True:
        lf, mf = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        ll = (0, int(rng.integers(1, 15)), int(rng.integers(15, 270)), _log_uniform(rng, 270, 1500))[lf]
        ml = (int(rng.integers(4, 19)), int(rng.integers(19, 274)), _log_uniform(rng, 274, 20000))[mf]
        if w.pos + ll + ml > target - 24:
            break
        w.seq(_rb(rng, ll), _draw_offset(rng, w.pos + ll, 65535), ml)
    w.last(_rb(rng, 5 if short else cap - w.pos))
    return w.finish(cap), w.expected


_cache = {}
CASES = _lz4_cases() + _snappy_cases()


def cases():
    return CASES


def random_streams():
    """[(codec, cap, [(stream, out)])]: 256 streams per codec at cap 65536 and 64 at cap 131072"""
    if "random" not in _cache:
        out = []
        for codec in ("lz4", "snappy"):
            for cap, n in ((65536, 256), (131072, 64)):
                rng = np.random.default_rng([len(codec), cap])
                out.append((codec, cap, [random_valid(codec, rng, cap) for _ in range(n)]))
        _cache["random"] = out
    return _cache["random"]


# ---------------------------------------------------------------------------------------------- frames
BLOCK = 65536
Frame = namedtuple("Frame", "codec name part frame out")   # the expected verdict is the restatement's (oracle_lib)


def _lz4f(blocks, linked: bool) -> bytes:
    """an LZ4 frame of 64 KiB blocks (lz4frame.c: magic, FLG, BD, header checksum; block size words; end mark)"""
    import oracle_lib as O
    hdr = bytes([0x40 | (0 if linked else 0x20), 0x40])
    h = np.frombuffer(hdr, np.uint8).copy()
    hc = (O.oracle().oracle_xxh32(h.ctypes.data, len(h), 0) >> 8) & 0xff
    body = b"".join(len(b).to_bytes(4, "little") + b for b in blocks)
    return (0x184D2204).to_bytes(4, "little") + hdr + bytes([hc]) + body + bytes(4)


def _nvlz4(blocks, n: int) -> bytes:
    """the nvcomp LZ4 container (oracle/frame_oracle.c): 4, metadata bytes, n, chunk size, k + 1 offsets"""
    k = len(blocks)
    m = (4 + k + 1) * 8
    offs, o = [], m
    for b in blocks:
        offs.append(o)
        o += len(b)
    offs.append(o)
    return b"".join(v.to_bytes(8, "little") for v in [4, m, n, BLOCK] + offs) + b"".join(blocks)


def linked_second_block(rng, first_out: bytes):
    """(stream, output) of a full block decoded after first_out: matches that start in the previous block and run
    into this one, as group members and through the checked path, then sources anywhere in both blocks"""
    w = Lz4Writer(prefix=first_out)
    w.seq(b"", 3, 40)                                     # starts 3 bytes before the block, overlaps into it
    w.seq(_rb(rng, 2), w.pos + 2 + 10, 18)                # ... and 10 bytes before it, after literals
    w.seq(_rb(rng, 9), w.pos + 9 + 1, 700)                # the checked path
    w.seq(b"", 65535, 15)
    w.seq(_rb(rng, 300), w.pos + 300 + 200, 150)          # 200 bytes before the block, not into it
    while w.pos < BLOCK - 3000:
        ll = int(rng.integers(0, 40))
        w.seq(_rb(rng, ll), _draw_offset(rng, min(w.pos + ll + BLOCK, 65535), 65535), int(rng.integers(4, 300)))
    w.last(_rb(rng, BLOCK - w.pos))
    return w.finish(BLOCK), w.expected


def frames():
    """frames of two full 64 KiB blocks each: independent blocks, linked blocks (block 2 reads block 1), nvcomp
    containers; one frame of each kind whose second block is a rejected stream"""
    if "frames" in _cache:
        return _cache["frames"]
    rng = np.random.default_rng(20263)
    full = [(c.stream, c.out) for c in cases() if c.codec == "lz4" and c.cap == BLOCK and c.ok and len(c.out) == BLOCK]
    full += [(s, o) for codec, cap, lst in random_streams() if codec == "lz4" and cap == BLOCK for s, o in lst
             if len(o) == BLOCK][:32]
    bad = next(c.stream for c in cases() if c.name == "limit-cap-5-late-past")
    out = []
    for i in range(0, len(full) - 1, 2):
        (s0, o0), (s1, o1) = full[i], full[i + 1]
        out.append(Frame("lz4f", f"independent-{i}", 2 * BLOCK, _lz4f([s0, s1], False), o0 + o1))
        out.append(Frame("nvlz4", f"container-{i}", 2 * BLOCK, _nvlz4([s0, s1], 2 * BLOCK), o0 + o1))
    for i, (s0, o0) in enumerate(full[:12]):
        s1, o1 = linked_second_block(rng, o0)
        out.append(Frame("lz4f", f"linked-{i}", 2 * BLOCK, _lz4f([s0, s1], True), o0 + o1))
    s0, o0 = full[0]
    out.append(Frame("lz4f", "independent-bad-block", 2 * BLOCK, _lz4f([s0, bad], False), None))
    out.append(Frame("lz4f", "linked-bad-block", 2 * BLOCK, _lz4f([s0, bad], True), None))
    out.append(Frame("nvlz4", "container-bad-block", 2 * BLOCK, _nvlz4([s0, bad], 2 * BLOCK), None))
    _cache["frames"] = out
    return out
