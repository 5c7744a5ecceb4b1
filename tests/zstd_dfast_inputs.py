"""tests/zstd_dfast_inputs.py -- small named, seeded inputs that steer zstd's level-3 (double-fast) parser into the
events of tests/zstd_dfast_census.py that the corpora reach only by chance or never; each is one frame.
tests/test_zstd_dfast_census.py holds every input to the classes it declares and anchors the host walk to the
reference build on it; tests/test_gpu_zstd_dfast_census.py runs them through every level-3 GPU compress path against
the digests of tests/golden/zstd_dfast_census_golden.json (tests/golden/make_zstd_dfast_census_golden.py).

How the inputs steer the parser:
  dense(pieces)      a random head (a search's first 256 positions step by 1, so each of them is in both tables),
                     then for each (lit, m, src): lit fresh random bytes and a copy of the m bytes at head position src.
                     The byte before a copy differs from the byte before its source (no catch-up) and the byte after
                     it from the byte after the source's end, so the literal run is exactly lit and the match exactly
                     m, found by the long table at the copy's first byte.  lit 256 puts the copy on the first position
                     searched at a step of 2.
  nseq(k)            dense with k pieces of 9 literals and a 24-byte copy: a block of exactly k sequences, for the
                     table-type thresholds of ZSTD_selectEncodingType (32 and 64 at strategy 2; 36 and 72 at 1)
  late(head, m)      head random bytes, then a copy of m bytes from the head's dense start.  The search reaches the
                     copy at a step of 1 + head / 256 and finds it some bytes in; the catch-up goes back to the copy's
                     first byte.  The head lengths below were picked so that the catch-up is exactly 64 bytes and more than 64,
                     and so that a step of 3 and of 4 (no hl1 insertion) finds the match.
  lit65536           late() with 65,600 random 7-bit bytes (compressible literals, no matches) before the first match of
                     a one-block frame: the literal-length escape
  sevenbit3000       random 7-bit bytes: no match, Huffman-compressible literals: a compressed block of no sequences
  ll-rle             dense with every literal run in 128..255 and every match 24 bytes: LL and ML tables of one symbol
  periods            offsets 2..7: the 8-byte loads of source and target overlap
  twins              the same kinds just over 16384 bytes take the mls 5 row (hash_short over 5 bytes)
  corpus slices      small text / json / runs / zero inputs of one, two and three blocks for the events that need
                     ordinary redundancy (repcodes, short matches, the long match at ip + 1) or a second block
  far_copy           tests/zstd_dfast_cases.py's 2.5 MiB input, the only one whose window slides (stale indexes)"""
from typing import Callable, NamedTuple

import numpy as np

import zstd_dfast_cases as Z


class Inp(NamedTuple):
    name: str
    make: Callable[[], np.ndarray]
    classes: tuple                          # classes of tests/zstd_dfast_census.py this input is there for


def _rng(seed):
    return np.random.default_rng(seed)


def _other(rng, *avoid):
    while True:
        b = int(rng.integers(0, 256))
        if b not in avoid:
            return b


def dense(seed, pieces, head=240, tail=24, pad=0):
    """see the module's docstring; pad: random bytes appended (to pass a size threshold)"""
    def make():
        rng = _rng(seed)
        need = max([src + m + 1 for _, m, src in pieces] + [head])
        out = rng.integers(0, 256, need, dtype=np.uint8).tolist()
        stop = None
        for lit, m, src in pieces:
            fresh = rng.integers(0, 256, lit, dtype=np.uint8).tolist()
            if lit == 1:
                fresh[0] = _other(rng, stop, out[src - 1])
            elif lit:
                fresh[0] = _other(rng, stop)
                fresh[-1] = _other(rng, out[src - 1])
            out += fresh
            out += out[src:src + m]
            stop = out[src + m]
        out.append(_other(rng, stop))
        out += rng.integers(0, 256, tail, dtype=np.uint8).tolist()
        out += rng.integers(0, 128, pad, dtype=np.uint8).tolist()     # (7-bit bytes: the frame stays compressible)
        return np.array(out, np.uint8)
    return make


def nseq(k, pad=0):
    return dense(1000 + k, [(9, 24, 4 + 3 * i) for i in range(k)], pad=pad)


def late(seed, head, m, src=8, top=256):
    def make():
        rng = _rng(seed)
        h = rng.integers(0, top, head, dtype=np.uint8)
        h[-1] = _other(rng, int(h[src - 1]))
        t = rng.integers(0, 256, 40, dtype=np.uint8)
        t[0] = _other(rng, int(h[src + m]))
        return np.concatenate([h, h[src:src + m], t])
    return make


def period(p, n=3000):
    return lambda: np.resize(_rng(100 + p).integers(0, 256, p, dtype=np.uint8), n)


def corpus(kind, n, seed=Z.SEED):
    return lambda: Z.corpus(kind, n, seed)


FAR = "far_copy"
_COUNTS = (255, 256, 257, 511, 512, 600)     # bytes matched past the 8-byte seed
_LITS = (1, 63, 64, 65, 255, 256, 257, 300)
_NSEQ = (31, 32, 33, 36, 37, 63, 64, 65, 72, 73)

INPUTS = [
    Inp("counts", dense(21, [(9, 8 + c, 10 + 3 * i) for i, c in enumerate(_COUNTS)], head=700),
        ("count/1-255", "count/256", "count/257-511", "count/512+", "search/long-hit", "catchup/0")),
    Inp("counts-mls5", dense(21, [(9, 8 + c, 10 + 3 * i) for i, c in enumerate(_COUNTS)], head=700, pad=16384),
        ("count/256", "count/512+", "params/mls5")),
    Inp("lits", dense(22, [(lit, 24, 6 + 5 * i) for i, lit in enumerate(_LITS)]),
        ("lit/1-63", "lit/64", "lit/65-255", "lit/256", "lit/>256", "step/2", "params/mls4")),
    Inp("lits-mls5", dense(22, [(lit, 24, 6 + 5 * i) for i, lit in enumerate(_LITS)], pad=16384),
        ("lit/64", "lit/256", "lit/>256", "step/2", "params/mls5")),
    Inp("step3", late(31, 700, 200), ("step/3", "post/hl1-inserted")),
    Inp("step4", late(32, 1100, 200), ("step/4+", "post/hl1-skipped")),
    Inp("catchup64", late(33, 18237, 400), ("catchup/64", "step/4+")),
    Inp("catchup70", late(34, 19025, 400), ("catchup/65+", "step/4+")),
    Inp("lit65536", late(77, 65600, 600, top=128), ("lit/>=65536", "catchup/65+", "params/row/n<=131072")),
] + [
    Inp(f"nseq{k}", nseq(k), (f"nseq/{k}",)) for k in _NSEQ
] + [
    Inp(f"nseq{k}-mls5", nseq(k, pad=16384), (f"nseq/{k}", "params/mls5")) for k in (32, 64)
] + [
    Inp(f"period{p}", period(p), ("off/1",) if p == 1 else ("off/2-7",)) for p in (1, 2, 3, 4, 5, 6, 7)
] + [
    Inp("period3-17000", period(3, 17000), ("off/2-7", "params/mls5")),
    Inp("zero70000", corpus("zero", 70000), ("ml/>=65539-rep", "off/1", "count/to-block-end")),
    Inp("zero140000", corpus("zero", 140000), ("frame/blocks/2", "block/repcodes-unconfirmed")),
    Inp("text9", corpus("text", 9), ("block/too-short-to-search", "params/wlog-raised-to-10")),
    Inp("text5", corpus("text", 5), ("block/under-7-bytes",)),
    Inp("text5000", corpus("text", 5000), ("search/rep-hit", "search/short-kept", "search/long-at-ip+1",
                                           "hit/fresh-long")),
    Inp("json17000", corpus("json", 17000), ("params/mls5", "imm-rep/2+", "search/long-at-ip+1")),
    Inp("runs40000", corpus("runs", 40000), ("off/1", "imm-rep/2+", "hit/fresh-short")),
    Inp("sevenbit3000", lambda: _rng(55).integers(0, 128, 3000, dtype=np.uint8), ("block/no-sequences", "search/ran-out")),
    Inp("ll-rle", dense(41, [(150, 24, 4 + 3 * i) for i in range(5)], head=100), ("lit/65-255", "search/long-hit")),
    Inp("random3000", corpus("random", 3000), ("block/no-sequences", "search/ran-out", "block/saved-restored")),
    Inp("text131080", corpus("text", 131080), ("frame/blocks/2", "block/later", "block/too-short-to-search")),
    Inp("text140000", corpus("text", 140000), ("frame/blocks/2", "off/earlier-block", "imm-rep/1")),
    Inp("period3-70000", period(3, 70000), ("ml/>=65539", "off/2-7")),
    Inp("mixed270000", corpus("mixed", 270000), ("frame/blocks/3+", "params/row/n>262144", "off/>=65536")),
    Inp("raw-block-then-text", corpus("random_block_then_text", 131072 + 30000),
        ("block/repcodes-unconfirmed", "frame/blocks/2")),
    Inp(FAR, corpus("far_copy_then_near_copy", 2400 * 1024 + 517 + 2 * 65536),
        ("block/dl>0", "block/plow>dl", "reject/long/stale", "reject/short/stale")),
]

BY_NAME = {i.name: i for i in INPUTS}
assert len(BY_NAME) == len(INPUTS)


if __name__ == "__main__":          # python tests/zstd_dfast_inputs.py DIR: one file per input (for the walk program)
    import os
    import sys
    for inp in INPUTS:
        inp.make().tofile(os.path.join(sys.argv[1], inp.name + ".bin"))
