"""tests/zstd_dict_frames.py -- valid zstd frames built by hand for the dictionary decoder (include/lzbench_hip.h 3f:
zstdd::decode_block's DictT and zdd::DictSrc), one named frame per path a sequence can take whose source starts in
the dictionary, beside tests/zstd_hand_frames.py and with its pieces: RLE-coded sequence tables (one code each per
block, so a block's sequences share one literal-length, one offset and one match-length code, and a frame takes
several blocks where it needs offsets or lengths of other magnitudes).

The model (Builder) executes what it writes over `dictionary + content so far`, with the repeat offsets of RFC 8878
3.1.1.5 as zstd 1.5.2's ZSTD_decodeSequence applies them: offset codes 0 and 1, the shift by one where the literal
length is 0, rep0 - 1, an offset of 0 forced to 1, the start values 1, 4, 8, carried from block to block.  A sequence
whose offset reaches before the dictionary's first byte raises Reject; the same frame built over a shorter dictionary
is how a rejecting case gets its verdict.  Expected content comes from the model alone; the reference build, where
present, must agree frame by frame (tests/test_zstd_dict_frames.py).

Builder.trace lists what the decoder executes: Ev(pos, ll, ml, off, rep, blk) per sequence (pos: the content position
where its literals start; rep: the offset came from a repeat code; blk: the block's index), and the same with ml = 0
for a raw block and for a block's last literals.  classify() names the decoder's cases over such a trace, from the
thresholds of lzbench_amd/csrc/zstdd.h: the 2 KiB LDS output window (kZW), a window match's reach (kZW - 128),
literal runs above 512 bytes that bypass the window (and move ringlo), copy rounds of 64 bytes."""
from collections import namedtuple

import numpy as np

import lzbench_amd as L
import zstd_hand_frames as H

KZW, REACH, BULK, ROUND = 2048, 2048 - 128, 512, 64
ND = 5003                                   # the dictionary of every frame here
Ev = namedtuple("Ev", "pos ll ml off rep blk")

EVENTS = ("dict/whole", "dict/straddle/period", "dict/straddle/window", "dict/straddle/far", "dict/straddle/far-overlap",
          "dict/first-byte", "dict/copy>64", "dict/copy>window", "dict/rep", "dict/after-bulk", "dict/after-group",
          "dict/before-group", "dict/long-literals")


class Reject(ValueError):
    pass


def dictionary() -> np.ndarray:
    return L.datagen("random", ND, seed=8301).copy()


def _code(table, n):
    c = max(k for k, (base, _) in table.items() if base <= n)
    assert n - table[c][0] < (1 << table[c][1]) or (table[c][1] == 0 and n == table[c][0]), n
    return c, n - table[c][0]


def header(n: int, did=None, single=True) -> bytes:
    """frame header with a 4-byte content size; did: a dictionary-ID field of one byte; single=False: a window
    descriptor (the smallest power of two that holds the content, 1 KiB at least) ahead of it"""
    fhd = (2 << 6) | (0x20 if single else 0) | (0 if did is None else 1)
    h = b"\x28\xb5\x2f\xfd" + bytes([fhd])
    if not single:
        h += bytes([(max(10, (max(n, 1) - 1).bit_length()) - 10) << 3])
    if did is not None:
        h += bytes([did])
    return h + n.to_bytes(4, "little")


class Builder:
    def __init__(self, d, seed=1):
        self.d = bytes(memoryview(np.ascontiguousarray(d)))
        self.hist = bytearray(self.d)
        self.rep = [1, 4, 8]
        self.blocks, self.trace = [], []
        self._pool = L.datagen("random", 16384, seed=8400 + seed).tobytes()
        self._at = 0

    @property
    def pos(self):
        return len(self.hist) - len(self.d)

    def fresh(self, n: int) -> bytes:
        """n seeded random bytes no earlier call returned"""
        assert self._at + n <= len(self._pool)
        self._at += n
        return self._pool[self._at - n: self._at]

    def raw(self, n: int):
        data = self.fresh(n)
        self.trace.append(Ev(self.pos, n, 0, 0, False, len(self.blocks)))
        self.hist += data
        self.blocks.append((0, n, data))

    def cmp(self, seqs, tail=0, reserved=0):
        """A compressed block of raw literals.  seqs: [(ll, ml, of)] with of an offset (a new one) or ("rep", code,
        extra bit) for the offset codes 0 and 1; tail: last literals; reserved: the mode byte's two low bits."""
        lits, extras, codes = b"", [], None
        blk = len(self.blocks)
        for ll, ml, of in seqs:
            llc, lle = _code(H.LL, ll)
            mlc, mle = _code(H.ML, ml)
            if isinstance(of, tuple):
                _, ofc, ofe = of
                assert ofc in (0, 1) and ofe < (1 << ofc)
            else:
                ofc = (of + 3).bit_length() - 1
                ofe = of + 3 - (1 << ofc)
                assert of > 0 and ofc >= 2
            assert codes in (None, (llc, ofc, mlc)), "one code each per block (RLE tables)"
            codes = (llc, ofc, mlc)
            extras.append((lle, ofe, mle))
            # ---- the model: ZSTD_decodeSequence's offset, ZSTD_execSequence's copy
            value = (1 << ofc) + ofe
            r = self.rep
            if value > 3:
                off, self.rep = value - 3, [value - 3, r[0], r[1]]
            else:
                idx = value - 1 + (ll == 0)
                if idx == 0:
                    off = r[0]
                elif idx == 1:
                    off, self.rep = r[1], [r[1], r[0], r[2]]
                elif idx == 2:
                    off, self.rep = r[2], [r[2], r[0], r[1]]
                else:
                    off = r[0] - 1 or 1
                    self.rep = [off, r[0], r[1]]
            self.trace.append(Ev(self.pos, ll, ml, off, value <= 3, blk))
            lit = self.fresh(ll)
            lits += lit
            self.hist += lit
            if off > len(self.hist):
                raise Reject(f"offset {off} at position {self.pos} with a dictionary of {len(self.d)} bytes")
            for _ in range(ml):
                self.hist.append(self.hist[-off])
        if tail:
            self.trace.append(Ev(self.pos, tail, 0, 0, False, blk))
            lit = self.fresh(tail)
            lits += lit
            self.hist += lit
        n = len(lits)
        body = H.literals_header(0, n, 1 if n < 32 else 2 if n < 4096 else 3) + lits
        s = bytearray(H.sequences(*codes, extras))
        s[1] |= reserved
        body += bytes(s)
        self.blocks.append((2, len(body), body))

    def frame(self, **hdr):
        content = bytes(self.hist[len(self.d):])
        f = header(len(content), **hdr)
        for i, (t, size, body) in enumerate(self.blocks):
            f += H.block(t, size, body, i == len(self.blocks) - 1)
        assert len(f) != len(content), "a frame as long as its content reads as stored raw"
        return f, content


# ---- the frames: name -> function(Builder) -> header arguments -------------------------------------------------
def _whole_short(b):
    b.cmp([(0, 40, 100)], tail=20)


def _whole_multi_round(b):
    b.cmp([(0, 200, 300)], tail=9)


def _whole_wrap(b):
    """2100 and 4500 bytes of the dictionary: more than the window, more than twice the window"""
    b.cmp([(0, 2100, 4000)], tail=3)
    b.cmp([(5, 4500, b.pos + 5 + 4800)])


def _dict_first_byte(b):
    b.cmp([(7, ND, 7 + ND)], tail=11)


def _straddle_period(back, ll=0, ml=100):
    def f(b):
        b.cmp([(ll, ml, ll + back)], tail=5)
    return f


def _straddle_window(b):
    b.raw(128)
    b.cmp([(0, 400, 128 + 40)], tail=1)


def _straddle_far(b):
    """a bulk raw block, then a match longer than its offset from 40 bytes before the dictionary's end"""
    b.raw(3000)
    b.cmp([(0, 3500, 3000 + 40)])


def _straddle_far_reach(b):
    """the same past the window's reach with ringlo at 0: four raw blocks of 500 bytes, none of them bulk"""
    for _ in range(4):
        b.raw(500)
    b.cmp([(0, 300, 2000 + 40)], tail=2)


def _after_bulk_literals(b):
    b.cmp([(600, 200, 600 + 30)], tail=4)


def _group_dict_group(back):
    def f(b):
        b.raw(300)
        b.raw(300)
        seqs = [(16, 35, 520), (17, 36, 509), (16, 36, 600)]
        at = 600 + sum(ll + ml for ll, ml, _ in seqs)
        seqs.append((17, 36, at + 17 + back))                      # the dictionary's; offset code 9 reaches 1020
        seqs += [(16, 35, 700), (17, 35, 509), (16, 36, at + 100)]
        b.cmp(seqs, tail=6)
    return f


def _initial_rep(code, bit, ml=30):
    def f(b):
        b.cmp([(0, ml, ("rep", code, bit))], tail=7)
    return f


def _rep_across_blocks(b):
    b.cmp([(64, 100, 300)])                                        # rep0 = 300, 236 bytes into the dictionary
    b.cmp([(70, 110, ("rep", 0, 0)), (64, 99, ("rep", 0, 0))], tail=3)   # at 234: the dictionary; at 408: the output


def _reserved_plain(bits):
    def f(b):
        b.raw(128)
        b.cmp([(3, 50, 90)], tail=2, reserved=bits)
    return f


def _reserved_dict(b):
    b.cmp([(3, 50, 90)], tail=2, reserved=2)


def _dict_id(did):
    def f(b):
        b.cmp([(2, 40, 100)], tail=20)
        return {"did": did}
    return f


def _window_descriptor(b):
    b.raw(100)
    b.cmp([(0, 300, 100 + 70)], tail=20)
    return {"single": False}


def _long_literals_then_dict(b):
    b.cmp([(300, 100, 300 + 50)], tail=8)


FRAMES = {
    "whole-short": _whole_short,
    "whole-multi-round": _whole_multi_round,
    "whole-wrap": _whole_wrap,
    "dict-first-byte": _dict_first_byte,
    "straddle-period-2": _straddle_period(2),
    "straddle-period-1": _straddle_period(1),
    "straddle-period-37": _straddle_period(32, ll=5, ml=300),
    "straddle-window": _straddle_window,
    "straddle-far": _straddle_far,
    "straddle-far-reach": _straddle_far_reach,
    "after-bulk-literals": _after_bulk_literals,
    "group-dict-group": _group_dict_group(200),
    "group-straddle-group": _group_dict_group(30),
    "initial-rep1": _initial_rep(0, 0),
    "initial-rep2": _initial_rep(1, 0),
    "initial-rep0-minus-1": _initial_rep(1, 1),
    "rep-across-blocks": _rep_across_blocks,
    "reserved-bit0-plain": _reserved_plain(1),
    "reserved-bit1-dict": _reserved_dict,
    "dict-id-zero": _dict_id(0),
    "dict-id-nonzero": _dict_id(0x2A),
    "window-descriptor": _window_descriptor,
    "long-literals-then-dict": _long_literals_then_dict,
}
NEEDS_NO_DICTIONARY = ("reserved-bit0-plain",)
# (name, the dictionary's bytes dropped at its front): the calls that must give a negative status
REJECTS = (("dict-first-byte", 1), ("dict-id-nonzero", 1))


def build(name, d, fn=None):
    """(frame, content, trace) of a named frame over dictionary d; raises Reject where a sequence reaches before d;
    fn: another function in the named frame's place, over the same literals"""
    b = Builder(d, seed=sorted(FRAMES).index(name))
    hdr = (fn or FRAMES[name])(b) or {}
    f, content = b.frame(**hdr)
    return f, content, b.trace


def expected(name, d):
    """(status, content) of decoding the frame written over the full dictionary with d in its place"""
    if name == "dict-id-nonzero":
        return -1, b""                      # raw content has dictionary ID 0: any other ID in the header is another's
    try:
        _, content, _ = build(name, d)
    except Reject:
        return -1, b""
    return len(content), content


_cache = {}


def frames():
    """[(name, frame, content, trace)] over dictionary(), built once"""
    if "all" not in _cache:
        d = dictionary()
        _cache["all"] = [(n, *build(n, d)) for n in FRAMES]
    return _cache["all"]


def reserved_plain_cleared():
    """reserved-bit0-plain with its reserved bit cleared: (frame, content), the content the same"""
    f, content, _ = build("reserved-bit0-plain", dictionary(), _reserved_plain(0))
    return f, content


def accepting():
    return [f for f in frames() if f[0] != "dict-id-nonzero"]


# ---- the classifier ---------------------------------------------------------------------------------------------
def _big(e, far):
    return e.ll > 255 or e.ml > 4095 or far


def classify(trace, nd):
    """[(index into trace, set of event names)] for the sequences of a trace whose source starts in a dictionary of
    nd bytes"""
    out, ringlo = [], 0
    for i, e in enumerate(trace):
        at = e.pos + e.ll
        if e.ll > BULK:
            ringlo = at
        if not e.ml or e.off <= at:
            continue
        back = e.off - at
        dn = min(back, e.ml)
        names = set()
        if dn == e.ml:
            names.add("dict/whole")
        else:
            windowed = ringlo == 0 and e.off <= REACH
            if windowed:
                names.add("dict/straddle/period" if e.off < ROUND else "dict/straddle/window")
            else:
                names.add("dict/straddle/far")
                if e.ml - dn > e.off:
                    names.add("dict/straddle/far-overlap")
            if ringlo:
                names.add("dict/after-bulk")
        if back == nd:
            names.add("dict/first-byte")
        if dn > ROUND:
            names.add("dict/copy>64")
        if dn > KZW:
            names.add("dict/copy>window")
        if e.rep:
            names.add("dict/rep")
        if 255 < e.ll <= BULK:
            names.add("dict/long-literals")

        def grouped(j):
            o = trace[j] if 0 <= j < len(trace) else None
            return o is not None and o.blk == e.blk and o.ml and not _big(o, o.off > o.pos + o.ll)
        if grouped(i - 1):
            names.add("dict/after-group")
        if grouped(i + 1):
            names.add("dict/before-group")
        out.append((i, names))
    return out


def events(trace, nd):
    u = set()
    for _, names in classify(trace, nd):
        u |= names
    return u


def trace_of_walk(seqs, n):
    """the trace of the host walk's sequences (ll, ml, offBase) of a chunk of n bytes: one block, offBase 1 the only
    repeat code the fast strategy writes"""
    t, rep, pos = [], [1, 4, 8], 0
    for ll, ml, ob in seqs:
        ll, ml, ob = int(ll), int(ml), int(ob)
        if ob > 3:
            rep = [ob - 3, rep[0], rep[1]]
        else:
            assert ob == 1
            if ll == 0:
                rep = [rep[1], rep[0], rep[2]]
        t.append(Ev(pos, ll, ml, rep[0], ob <= 3, 0))
        pos += ll + ml
    if n > pos:
        t.append(Ev(pos, n - pos, 0, 0, False, 0))
    return t
