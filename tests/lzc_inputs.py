"""tests/lzc_inputs.py -- small named, seeded inputs that steer the LZ4 and snappy compressors into the parser
events (tests/lzc_census.py) that the corpora reach only by chance or never, each one chunk, with the levels it
runs at, its compressed size per level (the restatement's and the reference build's) and the classes it is there
for.  tests/test_lzc_census.py holds every row to its declaration on the CPU; tests/test_gpu_lzc_census.py runs the
rows through every GPU compress path.

How the inputs steer the parser:
  zeros / periods    one match at the period's offset to matchlimit; the sizes straddle n<13, the byU16/byU32 limit
                     and the former count cap (600000 zeros: a count of 599990)
  rep65535, rep65536 a random block of that many bytes twice and more, in a byU32 chunk: every candidate is exactly
                     65535 back (taken) or 65536 back (one too far: all literals, the search runs out)
  dense              (lits, matches, retests, count0) a short random head, every position of which is in the table,
                     then pieces of `lit` fresh bytes + a copy of `m` head bytes; the bytes around each copy differ
                     from those around its source, so the literal run is exactly `lit` and the match exactly `m`
  spliced            (sparse_source) copies out of a long random stretch that the search indexed sparsely: the hit
                     comes some bytes into the copy and catches up; lengths are not controlled
  accper(acc)        8 bytes, then a random block of acc + 1 bytes repeated.  A search from the start probes 1, 2,
                     2 + acc, 2 + 2 acc, ..: probes 1..64 cannot hit (their distances are no multiple of the period),
                     the 65th step is acc + 1 and the next probe hits its predecessor, with a catch-up back to byte 8:
                     about 64 acc bytes (acc 99, lzbench's highest lz4fast level: 6.3 KiB; acc 21845: 1.4 MB, past
                     4096 steps of the parse kernels' catch-up)
  catchup(k)         8 bytes, then a random block of 4 (6 + k) bytes repeated, at acceleration 6 + k: the probe at
                     2 + acc = 8 + k is the first inserted position of the periodic part, the hit is one period on and
                     catches up exactly k bytes, to the 8th byte (which differs)
  tostart            the same without the 8 bytes: the catch-up stops at the chunk's first byte
  zeros16m           16 MiB + 4096 zeros with noise islands: more than 16 MiB takes the fused kernel, whose own parse
                     counts and catches up
  snappy             fragments of every table size, chunk sizes around the fragment limit, and spliced pieces with the
                     copy lengths and offsets where EmitCopy changes shape and the literal lengths where the tag does"""
from typing import Callable, Dict, NamedTuple

import numpy as np


class Inp(NamedTuple):
    name: str
    codec: str                              # "lz4" (levels = accelerations; 1 = the lz4 row, else lz4fast) or "snappy"
    make: Callable[[], np.ndarray]
    levels: tuple
    packed: Dict[int, int]                  # level -> compressed bytes (restatement == reference build)
    classes: tuple                          # classes (without the codec prefix) reached at every level
    classes_at: Dict[int, tuple] = {}       # more, at one level


def _rng(seed):
    return np.random.default_rng(seed)


def _rand(seed, n):
    return _rng(seed).integers(0, 256, n, dtype=np.uint8)


def zeros(n):
    return lambda: np.zeros(n, np.uint8)


def period(p, n=3000):
    return lambda: np.resize(_rand(100 + p, p), n)


def repeat_block(block, n=200000):
    return lambda: np.resize(_rand(block, block), n)


def spliced(seed, pieces, head=600, tail=40):
    """head random bytes, then for each (lit, m, back): lit fresh random bytes, a copy of the m bytes `back` before
    the copy's start, and one byte that differs from the source's next.  Nothing is exact here: a literal run also
    holds the byte that ended the copy before it, the head is sparsely indexed (a long search steps ever wider), so
    a copy is found some bytes in and caught up (LZ4) or cut short (snappy).  For inputs that want such sources;
    exact lengths come from dense(), sn_copy() and sn_literal()."""
    def make():
        rng = _rng(seed)
        out = rng.integers(0, 256, head, dtype=np.uint8).tolist()
        for lit, m, back in pieces:
            fresh = rng.integers(0, 256, max(lit, 1), dtype=np.uint8).tolist()[:lit]
            at = len(out) + lit                  # the copy's start
            src = at - back
            assert src >= 1 and back >= 1
            if lit:
                fresh[-1] = (out + fresh)[src - 1] ^ 0xFF   # no catch-up past the copy's start
            out += fresh
            for i in range(m):
                out.append(out[src + i])
            out.append(out[src + m] ^ 0xFF)      # the match ends here
        out += rng.integers(0, 256, tail, dtype=np.uint8).tolist()
        return np.array(out, np.uint8)
    return make


def _other(rng, *avoid):
    while True:
        b = int(rng.integers(0, 256))
        if b not in avoid:
            return b


def dense(seed, pieces, head=56, tail=40, need=0):
    """LZ4 at acceleration 1: `head` random bytes (a search's first 64 probes step by 1, so every position of the
    head is in the table), then 3 fresh bytes and a copy of the 8 bytes at 50 (the first sequence, whose literals
    are the head), then for each (lit, m, src): lit fresh bytes and a copy of the m bytes at src, a head
    position under 50 that no other piece uses (a copy's own positions are not inserted, so the head's stay the
    candidates).
    The literal after a copy starts with a byte that ends the match, the one before a copy differs from the byte
    before its source: literal runs are exactly lit, matches exactly m.  A piece with lit 0 is found by the re-test.
    need: random bytes the sources read past the head."""
    def make():
        rng = _rng(seed)
        out = rng.integers(0, 256, max(head, need), dtype=np.uint8).tolist()
        stop = None                              # the byte that would continue the last match
        for lit, m, src in [(3, 8, 50)] + list(pieces):
            fresh = rng.integers(0, 256, lit, dtype=np.uint8).tolist()
            if lit == 1:
                fresh[0] = _other(rng, stop, out[src - 1])
            elif lit:
                fresh[0] = _other(rng, stop)
                fresh[-1] = _other(rng, out[src - 1])
            out += fresh
            for i in range(m):
                out.append(out[src + i])
            stop = out[src + m]
        out.append(_other(rng, stop))
        out += rng.integers(0, 256, tail, dtype=np.uint8).tolist()
        return np.array(out, np.uint8)
    return make


def toanchor():
    """a match that ends at e leaves e - 1 out of the table and e in it.  Later a match is followed at once by the
    bytes from e - 1 on: the re-test at its end misses, the search's first probe, one byte on, hits e and catches up
    one byte, to the anchor"""
    rng = _rng(31)
    out = rng.integers(0, 256, 60, dtype=np.uint8).tolist()
    out += [_other(rng, out[3])] * 5 + out[4:14]
    e = len(out)
    out += rng.integers(0, 256, 30, dtype=np.uint8).tolist()
    out += [_other(rng, out[19])] * 5 + out[20:30]
    out += out[e - 1: e + 24]
    out += [_other(rng, out[e + 24])] + rng.integers(0, 256, 40, dtype=np.uint8).tolist()
    return np.array(out, np.uint8)


def sn_copy(m, off):
    """snappy: 200 random bytes (a search's first 32 positions are all in the table), a run of zeros (one copy; the
    16 probes after a copy step by 1), 7 fresh bytes and a copy of the m bytes at 16, placed `off` after them; the
    bytes around it differ from those around its source.  snappy has no catch-up: the copy is found by the probe at
    its first byte or cut short."""
    def make():
        rng = _rng(1000 * off + m)
        c = 16 + off
        out = rng.integers(1, 256, 200, dtype=np.uint8).tolist() + [0] * (c - 207)
        out += [_other(rng, 0)] + rng.integers(0, 256, 5, dtype=np.uint8).tolist() + [_other(rng, out[15])]
        assert len(out) == c
        out += out[16:16 + m]
        out += [_other(rng, out[16 + m])] + rng.integers(0, 256, 40, dtype=np.uint8).tolist()
        return np.array(out, np.uint8)
    return make


def sn_literal(lit, m=0):
    """snappy: 20 random bytes, 60 zeros (one copy, which ends at the first byte that is not zero), `lit` bytes that
    are not zero, and with m a copy of the m bytes at 4 (in the table: a search's first 32 positions all are) and 40
    more bytes.  m = 0: the search after the zeros runs out, so the fragment ends with a literal of exactly lit.
    m > 0: the literal before the copy is exactly lit, which only some lengths can be: a literal that a copy follows
    starts where a search starts and ends at one of its probes (whose slot no fresh byte's hash may have taken: m
    picks the seed), at offsets 1..33, 35, .. 61, 63, 65, 68, .. 246,
    254, 262, 271 ..; so 61 and the neighbours of 256 (254, 262) are built this way, and 60, 256 and 257 can only
    end a fragment."""
    def make():
        rng = _rng(7000 + 10 * lit + m)
        out = rng.integers(1, 256, 20, dtype=np.uint8).tolist() + [0] * 60
        out += rng.integers(1, 256, lit, dtype=np.uint8).tolist()
        if m:
            out += out[4:4 + m]
            out += [_other(rng, out[4 + m], 0)] + rng.integers(1, 256, 40, dtype=np.uint8).tolist()
        return np.array(out, np.uint8)
    return make


def accper(acc, n, seed=7):
    def make():
        r = _rand(seed + acc, 8 + acc + 1)
        d = np.concatenate([r[:8], np.resize(r[8:], n - 8)])
        d[7] = d[7 + acc + 1] ^ 0xFF
        return d
    return make


def catchup(k, prefix=8):
    """(make, acceleration): a first hit that catches up exactly k bytes (prefix 8) or to the chunk's start (0)"""
    acc = 6 + k
    p = 4 * acc

    def make():
        r = _rand(50 + k + prefix, prefix + p)
        d = np.concatenate([r[:prefix], np.resize(r[prefix:], 3 * p + 64)])
        if prefix:
            d[prefix - 1] = d[prefix - 1 + p] ^ 0xFF
        return d
    return make, acc


def zeros16m():
    d = np.zeros((16 << 20) + 4096, np.uint8)
    for i, at in enumerate((5, 300000, 300100, 9000000, (16 << 20) + 100)):
        d[at: at + 40] = _rand(900 + i, 40)
    return d


BIG = (16 << 20) + 4096
# literal runs and match lengths of the spliced inputs (copies from 500 back: inside the random head)
_LITS = (14, 15, 16, 255, 256, 257, 269, 270, 271)
_MATCHES = (18, 19, 20, 23, 24, 25, 273, 274, 275, 279, 280)

LZ4_INPUTS = [
    Inp("zeros12", "lz4", zeros(12), (1, 2), {}, ("n<13", "table/byU16")),
    Inp("zeros13", "lz4", zeros(13), (1, 2), {}, ("hit/search", "off/1", "catchup/0", "count/to-matchlimit",
                                                   "end/match-at-mflimit", "last-literals/5", "count/1-19")),
    Inp("zeros17", "lz4", zeros(17), (1, 2), {}, ("off/1", "count/to-matchlimit")),
    Inp("zeros64", "lz4", zeros(64), (1, 2), {}, ("off/1", "count/21-275")),
    Inp("zeros65546", "lz4", zeros(65546), (1, 2), {}, ("table/byU16", "count/>275")),
    Inp("zeros65547", "lz4", zeros(65547), (1, 2), {}, ("table/byU32", "count/>275")),
    Inp("zeros600000", "lz4", zeros(600000), (1, 2), {}, ("table/byU32", "count/>262164", "count/to-matchlimit")),
] + [
    Inp(f"period{p}", "lz4", period(p), (1, 2), {}, (("off/1",) if p == 1 else ("off/2-3",) if p < 4 else ())
        + ("count/>275", "count/to-matchlimit"))
    for p in (1, 2, 3, 5, 63, 64, 65, 255)
] + [
    Inp("rep65535", "lz4", repeat_block(65535), (1, 2), {}, ("table/byU32", "off/65535")),
    Inp("rep65536", "lz4", repeat_block(65536), (1, 2), {}, ("table/byU32", "far/65536", "far/rejected",
                                                            "end/search-ran-out"), {1: ("step>1",), 2: ("step>acc",)}),
    Inp("lits", "lz4", dense(11, [(lit, 40, 4 + 5 * i) for i, lit in enumerate(_LITS)], need=100), (1,), {},
        ("lit/1-14", "lit/15", "lit/16-255", "lit/256+", "lit/270", "step>1", "catchup/1-3")),
    Inp("matches", "lz4", dense(12, [(9, m, 4 + 4 * i) for i, m in enumerate(_MATCHES)], need=340), (1,), {},
        ("ml/15", "ml/15+255", "count/1-19", "count/20", "count/21-275", "count/>275", "catchup/0")),
    Inp("retests", "lz4", dense(13, [(5, 8, 4)] + [(0, 6, 4 + 3 * i) for i in range(1, 12)]), (1,), {},
        ("hit/retest", "retest-chain>=8", "lit/0", "count/1-19")),
    Inp("count0", "lz4", dense(14, [(7, 4, 8), (0, 4, 20), (20, 4, 30)]), (1,), {}, ("count/0", "hit/retest")),
    Inp("toanchor", "lz4", toanchor, (1,), {}, ("catchup/to-anchor", "catchup/1-3")),
    Inp("sparse_source", "lz4", spliced(15, [(3, 400, 700), (30, 300, 1000)], head=2600), (1,), {},
        ("catchup/5-64", "step>1")),
    Inp("accper99", "lz4", accper(99, 8192), (99,), {}, ("step>acc", "catchup/>64", "count/to-matchlimit")),
    # (three 64 KiB blocks: as a linked frame the first block's catch-up runs in the linked-frame kernel)
    Inp("accper99x140k", "lz4", accper(99, 140000), (99,), {}, ("table/byU32", "step>acc", "catchup/>64")),
    Inp("zeros16m", "lz4", zeros16m, (1,), {}, ("count/>262164", "table/byU32")),
    Inp("accper21845", "lz4", accper(21845, BIG), (21845,), {}, ("step>acc", "catchup/>64", "count/>262164")),
]
for _k in (0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 300):
    _m, _a = catchup(_k)
    _c = "catchup/" + ("0" if _k == 0 else "1-3" if _k < 4 else "4" if _k == 4 else "5-64" if _k <= 64 else ">64")
    LZ4_INPUTS.append(Inp(f"catchup{_k}", "lz4", _m, (_a,), {}, (_c,)))
_m, _a = catchup(4, prefix=0)
LZ4_INPUTS.append(Inp("tostart", "lz4", _m, (_a,), {}, ("catchup/to-start",)))


def _frag(n, kind):
    """a chunk of n bytes: text-like (short words over a small alphabet: hits everywhere) or random"""
    def make():
        rng = _rng(n)
        if kind == "random":
            return rng.integers(0, 256, n, dtype=np.uint8)
        words = [bytes(rng.integers(97, 105, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(40)]
        s = b" ".join(words[int(i)] for i in rng.integers(0, 40, n // 3 + 8))
        return np.frombuffer(s[:n], np.uint8).copy()
    return make


_TABLE = {1: 256, 14: 256, 15: 256, 16: 256, 255: 256, 256: 256, 257: 512, 1000: 1024, 16383: 16384, 16384: 16384,
          65535: 16384, 65536: 16384, 65537: 16384}
_COPY_CLASS = {11: (), 12: ("copy2/len>=12",), 64: ("copy/64",), 65: ("copy/65-67",), 67: ("copy/65-67",),
               68: ("copy/68",), 131: (), 132: ("copy/>=132",)}

SNAPPY_INPUTS = [
    Inp(f"text{n}", "snappy", _frag(n, "text"), (0,), {},
        (f"table/{_TABLE[n]}",) + (("frag<15",) if n < 15 else ()) + (("frags/2",) if n > 65536 else ("frags/1",)))
    for n in sorted(_TABLE)
] + [
    Inp("text2000", "snappy", _frag(2000, "text"), (0,), {}, ("table/2048", "hit/search", "hit/retest", "copy1")),
    Inp("text3000", "snappy", _frag(3000, "text"), (0,), {}, ("table/4096",)),
    Inp("text5000", "snappy", _frag(5000, "text"), (0,), {}, ("table/8192",)),
    Inp("text64k14", "snappy", _frag(65536 + 14, "text"), (0,), {}, ("frag<15", "frags/2")),
    Inp("text300000", "snappy", _frag(300000, "text"), (0,), {}, ("frags/>=4",)),
    Inp("random3000", "snappy", _frag(3000, "random"), (0,), {}, ("probe>16", "probe/off>63", "search-ran-out",
                                                                   "lit/257-65536", "lit/remainder")),
    Inp("random65536", "snappy", _frag(65536, "random"), (0,), {}, ("search-ran-out", "lit/257-65536")),
    Inp("lit60", "snappy", sn_literal(60), (0,), {}, ("lit/1-60", "lit/remainder", "search-ran-out")),
    Inp("lit61", "snappy", sn_literal(61), (0,), {}, ("lit/61-256", "lit/remainder")),
    Inp("lit256", "snappy", sn_literal(256), (0,), {}, ("lit/61-256", "lit/remainder")),
    Inp("lit257", "snappy", sn_literal(257), (0,), {}, ("lit/257-65536", "lit/remainder")),
    Inp("lit61copy", "snappy", sn_literal(61, 30), (0,), {}, ("lit/61-256", "hit/search")),
    Inp("lit254copy", "snappy", sn_literal(254, 30), (0,), {}, ("lit/61-256", "hit/search")),
    Inp("lit262copy", "snappy", sn_literal(262, 31), (0,), {}, ("lit/257-65536", "lit>256-before-copy")),
    Inp("literal65536", "snappy", lambda: np.concatenate([_rand(23, 65536), np.resize(_rand(24, 7), 300)]), (0,), {},
        ("lit/257-65536", "frags/2", "copy2/len>=12")),
    Inp("zeros70000", "snappy", zeros(70000), (0,), {}, ("copy/>=132", "end/copy", "frags/2")),
]

SNAPPY_INPUTS += [
    Inp(f"copy{m}at{off}", "snappy", sn_copy(m, off), (0,), {},
        _COPY_CLASS[m] + ((("copy1",) if off == 2047 else ("copy2/off>=2048",)) if m == 11 else ()))
    for off in (2047, 2048) for m in sorted(_COPY_CLASS)
]

# compressed bytes per level, measured from the reference build (lz4 1.9.3 LZ4_compress_fast, snappy 1.1.8
# RawCompress); the restatement gives the same (tests/test_lzc_census.py checks both)
PACKED = {
    "zeros12": {1: 13, 2: 13}, "zeros13": {1: 10, 2: 10}, "zeros17": {1: 10, 2: 10}, "zeros64": {1: 11, 2: 11},
    "zeros65546": {1: 267, 2: 267}, "zeros65547": {1: 267, 2: 267}, "zeros600000": {1: 2363, 2: 2363},
    "period1": {1: 22, 2: 22}, "period2": {1: 23, 2: 23}, "period3": {1: 24, 2: 24}, "period5": {1: 26, 2: 26},
    "period63": {1: 85, 2: 85}, "period64": {1: 86, 2: 86}, "period65": {1: 87, 2: 87}, "period255": {1: 276, 2:
    276}, "rep65535": {1: 66329, 2: 66329}, "rep65536": {1: 200786, 2: 200786}, "lits": {1: 1819}, "matches":
    {1: 537}, "retests": {1: 147}, "count0": {1: 143}, "toanchor": {1: 153}, "sparse_source": {1: 2699},
    "accper99": {99: 150}, "accper99x140k": {99: 667}, "zeros16m": {1: 66051}, "accper21845": {21845: 87673}, "catchup0": {6: 43},
    "catchup1": {7: 47}, "catchup2": {8: 51}, "catchup3": {9: 55}, "catchup4": {10: 59}, "catchup5": {11: 63},
    "catchup6": {12: 67}, "catchup63": {69: 298}, "catchup64": {70: 302}, "catchup65": {71: 306}, "catchup300":
    {306: 1256}, "tostart": {10: 51}, "text1": {0: 3}, "text14": {0: 16}, "text15": {0: 17}, "text16": {0: 18},
    "text255": {0: 193}, "text256": {0: 202}, "text257": {0: 205}, "text1000": {0: 514}, "text16383": {0: 6280},
    "text16384": {0: 6184}, "text65535": {0: 21089}, "text65536": {0: 22428}, "text65537": {0: 21391},
    "text2000": {0: 894}, "text3000": {0: 1272}, "text5000": {0: 1832}, "text64k14": {0: 21637}, "text300000":
    {0: 99307}, "random3000": {0: 3005}, "random65536": {0: 65542}, "lit60": {0: 88}, "lit61": {0: 90}, "lit256": {0: 285}, "lit257": {0: 287}, "lit61copy": {0: 135}, "lit254copy": {0: 328}, "lit262copy": {0: 337}, "literal65536": {0:
    65565}, "zeros70000": {0: 3289}, "copy11at2047": {0: 352}, "copy12at2047": {0: 353}, "copy64at2047": {0:
    353}, "copy65at2047": {0: 355}, "copy67at2047": {0: 355}, "copy68at2047": {0: 355}, "copy131at2047": {0:
    358}, "copy132at2047": {0: 358}, "copy11at2048": {0: 353}, "copy12at2048": {0: 353}, "copy64at2048": {0:
    353}, "copy65at2048": {0: 356}, "copy67at2048": {0: 356}, "copy68at2048": {0: 356}, "copy131at2048": {0:
    359}, "copy132at2048": {0: 359}
}

INPUTS = [i._replace(packed=PACKED[i.name]) for i in LZ4_INPUTS + SNAPPY_INPUTS]
LZ4_INPUTS = [i for i in INPUTS if i.codec == "lz4"]
SNAPPY_INPUTS = [i for i in INPUTS if i.codec == "snappy"]


def rows():
    """(input, level) for every row"""
    return [(i, lv) for i in INPUTS for lv in i.levels]


def codec_of(inp, level):
    """the library's codec name of a row"""
    return "snappy" if inp.codec == "snappy" else ("lz4" if level == 1 else "lz4fast")
