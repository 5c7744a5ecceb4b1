"""tests/zstd_entropy_inputs.py -- small named, seeded inputs that steer the zstd entropy stage into the decisions
of tests/zstd_entropy_census.py, each one frame (its chunk is its size), with the classes it is there for (least
counts: the counts the restatement gives) and the frame's size per level, measured from the restatement and the
reference build (zstd 1.5.2).  tests/test_zstd_entropy_census.py holds every row to its declaration on the CPU;
tests/test_gpu_zstd_entropy_census.py runs the rows through the GPU compressors and decoders.  The rows named
"edge:NAME" and "dfast:NAME" at the table's end are rows of tests/zstd_edge_inputs.py (at their own chunk size and
recorded packed size) and inputs of tests/zstd_dfast_inputs.py (one frame) that carry a class no row built here
does; they are imported, not copied.

How the inputs steer the stage (literals at level 1 only: the negative levels store them raw):
  literals(hist)     a run with a chosen histogram in which no 4-byte window repeats: as an input of its own it is one
                     block of no sequences whose literals are the run.  Tried here for the first time: the greedy draw
                     works for flat histograms (lit63, lit64) and gets stuck on skewed ones over few symbols, where a
                     window must repeat; those use separators()
  separators(seps)   the technique of zstd_edge_inputs' rle_literals with chosen separator bytes: block 2's literals
                     are the separators, whatever their histogram; with skewed() as block 1 the block before leaves a
                     Huffman table with codes of 5 and of 8-9 bits, and mix() picks how many separators have which
  pieces(parts)      a random head and (literals, copy) parts for exact literal lengths, match lengths and sequence
                     counts under the fast match finder (the level-1 counterpart of zstd_dfast_inputs.dense)
  periodic(mls)      runs of period 8: a block of exactly len(mls) sequences with literal length 8 and the match
                     lengths given, for a chosen match-length code histogram (ml_flat, m2_second_pass: each did
                     what its comment computes on the first seed)
  corpus rows        text / json / mixed / random slices for the decisions ordinary data takes
Search bounds: nseq63 .. nseq129 took the first seed of 100 k .. 100 k + 7 whose block has exactly k sequences (the
first one each time); old_table_mingain took the first of 100, 110 .. 250 frequent separators of 1000 whose streams
land in the 17 bytes between the size test and the gain test (190, 200 and 210 do; the row takes 200);
ratio19 / ratio20: literal runs of 6 and 7 bytes put literals / sequences at 194 / 10 and 204 / 10.  The searches
that found nothing are recorded with NOT_REACHED in tests/zstd_entropy_census.py."""
from typing import Callable, Dict, NamedTuple

import numpy as np

import lzbench_amd as L
import zstd_dfast_inputs as DI
import zstd_edge_inputs as E

BLOCK = E.BLOCK


class Row(NamedTuple):
    name: str
    make: Callable[[], np.ndarray]
    levels: tuple
    packed: Dict[int, int]                  # level -> the frame's bytes (restatement == reference build)
    classes: Dict[str, int]                 # class -> least count, at level 1 (literals are steered there only)
    at: Dict[int, Dict[str, int]] = {}      # level -> more classes, at that level
    chunk: int = 0                          # 0: one frame of the input's size (packed: the frame, no raw-store rule);
                                            # else the chunk size of lzbench's loop (packed: the packed stream)


def _rng(seed):
    return np.random.default_rng(seed)


def literals(seed, hist):
    """bytes with exactly the histogram {symbol: count} in which no 4-byte window occurs twice and no byte occurs
    five times in a row: the match finder compares 4 bytes at a candidate and at the repeat offset 1, so as an input
    of its own the run is one block of no sequences whose literals are the run.  A greedy draw without replacement
    that rejects a symbol completing a window already seen."""
    def make():
        rng = _rng(seed)
        left = dict(hist)
        out, seen = [], set()
        for _ in range(sum(hist.values())):
            syms = [s for s, c in left.items() if c > 0]
            w = np.array([left[s] for s in syms], float)
            for s in rng.choice(len(syms), size=len(syms), replace=False, p=w / w.sum()):
                b = syms[int(s)]
                win = tuple(out[-3:] + [b])
                if len(win) == 4 and (win in seen or (len(out) >= 4 and out[-4:] == [b] * 4)):
                    continue
                break
            else:
                raise AssertionError("no symbol fits: lower the skew")
            if len(win) == 4:
                seen.add(win)
            out.append(b)
            left[b] -= 1
        return np.array(out, np.uint8)
    return make


def flatish(n_sym, each, big, first=0):
    """{first .. first + n_sym - 1: each}, the first symbol `big` times instead"""
    h = {first + i: each for i in range(n_sym)}
    h[first] = big
    return h


def pieces(seed, parts, head=100, top=256):
    """a head of random bytes, every position of which the fast match finder indexes (a search's first 128 bytes go by
    in steps of 2 with both positions probed), then for each (lit, m) of parts: lit fresh random bytes and a copy of
    m bytes from a head position of its own (4 + i for part i: distinct first bytes), the head being as long as the
    longest copy needs.  The byte before a copy differs from the byte before its source and the byte after it from
    the byte after the source's end, so a part is one sequence of literal length lit and match length m, unless a
    later insertion has overwritten the source's slot in the hash table: the seeds below are ones where none has."""
    def make():
        rng = _rng(seed)
        need = max([4 + i + m + 1 for i, (_, m) in enumerate(parts)] + [head])
        out = rng.integers(0, top, need, dtype=np.uint8).tolist()
        stop = None
        for i, (lit, m) in enumerate(parts):
            src = 4 + i
            fresh = rng.integers(0, top, lit, dtype=np.uint8).tolist()
            if lit == 1:
                fresh[0] = DI._other(rng, stop, out[src - 1])
            elif lit:
                fresh[0] = DI._other(rng, stop)
                fresh[-1] = DI._other(rng, out[src - 1])
            out += fresh
            out += out[src:src + m]
            stop = out[src + m]
        out.append(DI._other(rng, stop))
        out += rng.integers(0, top, 24, dtype=np.uint8).tolist()
        return np.array(out, np.uint8)
    return make


def separators(seed, seps, base_lo=64, base_hi=255, tail=None, first=None):
    """two blocks.  The first is `first` (default: random bytes in [base_lo, base_hi)) and zeros to its end; the second
    is, for each byte of seps, that byte and a 16-byte slice of the first block's start (slices 17 apart), then
    `tail` (default: the last separator) to the block's end: every slice is found by its hash and extended back to
    the separator, which matches nothing, so the second block's literals are the separators and one tail byte
    (tests/zstd_edge_inputs.py `rle_literals`, with chosen separators)."""
    def make():
        rng = _rng(seed)
        n = len(seps)
        prefix = rng.integers(base_lo, base_hi, 8 + n * 17, dtype=np.uint8) if first is None else first()
        assert len(prefix) >= 8 + n * 17
        b1 = np.zeros(BLOCK, np.uint8)
        b1[:len(prefix)] = prefix
        b2 = np.full(BLOCK, seps[-1] if tail is None else tail, np.uint8)
        for i, s in enumerate(seps):
            a = 4 + i * 17
            b2[i * 17] = s
            b2[i * 17 + 1: (i + 1) * 17] = prefix[a: a + 16]
        return np.concatenate([b1, b2])
    return make


def periodic(seed, mls, lit=8):
    """for each m of mls: lit fresh random bytes and then those bytes again and again for m bytes more (a match of
    offset lit and length exactly m, found at its first byte: the byte before the run differs from the byte lit
    before it, the byte after the match breaks the period).  No head and no shared sources: the block has exactly
    len(mls) sequences, every literal length is lit, and the match lengths are the ones given, in order."""
    def make():
        rng = _rng(seed)
        out = []
        for m in mls:
            p = rng.integers(0, 256, lit, dtype=np.uint8).tolist()
            if out:
                p[0] = DI._other(rng, out[-lit])           # (the match before ends here)
                p[-1] = DI._other(rng, out[-1])            # (no catch-up into the literals)
            out += p
            out += [p[i % lit] for i in range(m)]
        out += [DI._other(rng, out[-lit])] + rng.integers(0, 256, 23, dtype=np.uint8).tolist()
        return np.array(out, np.uint8)
    return make


def skewed(seed, n):
    """n bytes, half of them from 64..79 and half from 80..254: as a block's literals they get a Huffman table (kept
    for the next block) in which the first sixteen have codes of about 5 bits and the others of 8 or 9"""
    def make():
        rng = _rng(seed)
        return np.where(rng.integers(0, 2, n) == 0, rng.integers(64, 80, n), rng.integers(80, 255, n)).astype(np.uint8)
    return make


def mix(seed, n, frequent):
    """n separator bytes for a block after skewed(): `frequent` of them from 64..79, the others from 80..254"""
    rng = _rng(seed)
    a = np.concatenate([rng.integers(64, 80, frequent), rng.integers(80, 255, n - frequent)])
    rng.shuffle(a)
    return [int(x) for x in a]


def shuffled(seed, hist):
    a = [s for s, c in hist.items() for _ in range(c)]
    _rng(seed).shuffle(a)
    return [int(x) for x in a]


def _bits57():
    """block 1 random (stored raw); block 2: 9000 random literals, a copy of 100000 bytes from block 1's eighth byte
    (offset 140064: code 17), ten literals and a second short copy: the first sequence is not the last, so it has
    state bits (predefined tables: 6 + 5 + 6) next to 13 + 16 + 17 extra bits"""
    r = _rng(57)
    b1 = r.integers(0, 256, BLOCK, dtype=np.uint8)
    lit = r.integers(0, 256, 9000, dtype=np.uint8)
    lit[-1] = (int(b1[7]) + 1) & 255
    mid = r.integers(0, 256, 10, dtype=np.uint8)
    tail = r.integers(0, 256, BLOCK, dtype=np.uint8)
    return np.concatenate([b1, np.concatenate([lit, b1[8:8 + 100000], mid, b1[20:60], tail])[:BLOCK]])


def _binary_chunk():
    """the fourth 64 KiB chunk of test_zstd_oracle's binary corpus: the one chunk of the committed digests whose
    literal-length counts take FSE_normalizeM2"""
    return np.ascontiguousarray(L.datagen("binary", 208953, 5)[196608:262144])


_FIRST = skewed(11, 8 + 1400 * 17)
# match lengths of the 48 codes 2 .. 49, twice each: 96 sequences whose most frequent code has 2 < 96 >> 5
_FLAT_ML = {m: 2 for m in list(range(5, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051,
                                               4099, 8195]}
# 27 match-length codes once and 3 of them 104 times: table log 6, 27 of 64 slots go to counts of 1, the rest's
# 311 / 37 is over lowOne = 7: FSE_normalizeM2 takes its second pass
_M2_ML = {5: 104, 6: 104, 7: 104, **{m: 1 for m in range(8, 35)}}
_RARE = {**{0: 60, 1: 60, 2: 60}, **{s: 2 for s in range(3, 35)}}

def edge_row(name, level, classes):
    """a row of tests/zstd_edge_inputs.py at one of its levels, with its own chunk size and recorded packed size"""
    e = next(e for e in E.EDGES if e.name == name)
    return Row("edge:" + name, e.make, (level,), {level: e.packed[level]}, classes if level == 1 else {},
               at={} if level == 1 else {level: classes}, chunk=e.chunk)


def dfast_row(name, packed, classes):
    """an input of tests/zstd_dfast_inputs.py as one frame at level 1 (packed: the restatement's frame)"""
    return Row("dfast:" + name, DI.BY_NAME[name].make, (1,), {1: packed}, classes)


ROWS = [
    Row('lit63', literals(1, flatish(8, 7, 14)), (1, -1), {1: 72, -1: 72},
        {'lit/gate/n<=63': 1, 'lit/gate/n=63': 1, 'block/raw/mingain': 1},
        at={-1: {'lit/off': 1}}),
    Row('lit64', literals(2, flatish(8, 7, 15)), (1, -1), {1: 42, -1: 73},
        {'lit/gate/n=64': 1, 'lit/hdr/3': 1, 'lit/streams/1': 1, 'huf/maxnb/5': 1, 'huf/maxnb/by-floor5': 1,
         'huf/limit/not-needed': 1, 'huf/weights/fse': 1, 'huf/weights/fse-too-large': 1,
         'huf/weights/odd-count': 1, 'huf/table/direct': 1, 'block/cmp/new-huf-table-kept': 1,
         'hufw/norm/fast': 1, 'hufw/norm/p<8-rounded-up': 2, 'hufw/ncount/zero-run/0': 1,
         'hufw/ncount/count>=threshold': 2}),
    Row('weights_gap', separators(4, shuffled(4, _RARE), first=_FIRST), (1,), {1: 20389},
        {'lit/repeat/invalid': 1, 'lit/hdr/5': 1, 'lit/streams/4': 1, 'huf/maxnb/7': 1, 'huf/maxnb/11': 1,
         'huf/maxnb/by-max11': 1, 'huf/maxnb/by-minbits': 1, 'huf/sort/bucket>=165': 1,
         'huf/sort/qsort-partitioned': 1, 'huf/table/fse': 2, 'seq/ns%64/1': 1, 'seq/ns/1': 1,
         'seq/ml>=65539': 2, 'seq/ofcode>=17': 1, 'block/repcodes-confirmed': 1, 'seqtab/norm/fast': 2,
         'seqtab/norm/low/+1': 3, 'seqtab/ncount/zero-run/0': 1, 'seqtab/ncount/zero-run/3+': 3,
         'seqtab/ncount/zero-run/24+': 1, 'seqtab/ncount/count>=threshold': 4, 'seqtab/ncount/flush-mid-run':
         2, 'hufw/ncount/zero-run/1-2': 1, 'hufw/ncount/zero-run/3+': 1, 'seq/LL/type/rle': 1,
         'seq/LL/type/rle-as-predef': 1, 'seq/OF/type/rle-as-predef': 1, 'seq/OF/type/fse': 1,
         'seq/OF/last-count-trick/not': 1, 'seq/OF/tablelog/6': 1, 'seq/ML/type/rle-as-predef': 1,
         'seq/ML/type/fse': 1, 'seq/ML/last-count-trick/not': 1, 'seq/ML/tablelog/7': 1}),
    Row('two_symbols', separators(5, [0, 1] * 36, first=_FIRST), (1,), {1: 20289},
        {'huf/maxnb/by-srcsize': 1, 'huf/weights/wn<=1': 1, 'seqtab/norm/p<8-rounded-up': 1}),
    Row('weights_distinct', separators(3, shuffled(3, {0: 27, 1: 18, 2: 10, 3: 8}), tail=0), (1,), {1: 1234},
        {'lit/flat/raw': 1, 'huf/weights/all-distinct': 1, 'seq/ns/65': 1, 'seq/bits/>=32': 2,
         'seq/LL/type/predef-by-count': 1, 'seq/OF/last-count-trick/taken': 1, 'seq/ML/type/predef-by-count':
         1}),
    Row('old_table_too_large', separators(7, mix(7, 300, 0), first=_FIRST), (1,), {1: 20580},
        {'lit/repeat/small-direct': 1, 'lit/raw/streams-too-large/old': 1}),
    Row('old_table_by_estimate', separators(8, mix(8, 1400, 700), first=_FIRST), (1,), {1: 21483},
        {'lit/repeat/old-by-estimate': 1, 'lit/hdr/4': 1, 'huf/maxnb/9': 1, 'huf/limit/fired': 1,
         'huf/limit/repay/dec>1': 4, 'hufw/norm/low/+1': 2, 'seq/OF/tablelog/8': 1, 'seq/ML/tablelog/8': 1}),
    Row('new_table', separators(9, shuffled(9, {64: 700, 65: 400, 66: 200, 67: 100}), first=_FIRST), (1,), {1: 20622},
        {'lit/repeat/new-table': 1}),
    Row('old_table_mingain', separators(10, mix(10, 1000, 200), first=_FIRST), (1,), {1: 21283},
        {'lit/raw/mingain': 1, 'seq/OF/tablelog/7': 1}),
    Row('ll_last_unique', pieces(0, [(1 + (i & 1), 8) for i in range(80)] + [(9, 8)]), (1, -1), {1: 408, -1: 408},
        {'lit/raw/streams-too-large/new': 1, 'seqtab/ncount/zero-run/1-2': 2, 'seq/LL/type/fse': 1,
         'seq/LL/last-count-trick/not': 1, 'seq/LL/tablelog/6': 1, 'seq/OF/tablelog/5': 1,
         'seq/ML/last-count-trick/taken': 1, 'seq/ML/tablelog/5': 1}),
    Row('nseq63', pieces(6300, [(9, 24)] * 63), (1,), {1: 863},
        {'seq/ns/63': 1}),
    Row('nseq64', pieces(6400, [(9, 24)] * 64), (1, -1), {1: 874, -1: 874},
        {'seq/ns%64/0': 1, 'seq/ns/64': 1}),
    Row('nseq65', pieces(6500, [(9, 24)] * 65), (1,), {1: 886},
        {'seq/ns/65': 1, 'seq/ns%64/1': 1}),
    Row('nseq66', pieces(6600, [(9, 24)] * 66), (1,), {1: 897},
        {'seq/ns%64/2': 1}),
    Row('nseq67', pieces(6700, [(9, 24)] * 67), (1,), {1: 908},
        {'seq/ns%64/3': 1}),
    Row('nseq68', pieces(6800, [(9, 24)] * 68), (1,), {1: 920},
        {'seq/ns%64/4': 1}),
    Row('nseq69', pieces(6900, [(9, 24)] * 69), (1,), {1: 931},
        {'seq/ns%64/5': 1}),
    Row('nseq128', pieces(12800, [(9, 24)] * 128), (1,), {1: 1500},
        {'seq/ns/128': 1, 'seq/LL/last-count-trick/taken': 1, 'seq/ML/tablelog/6': 1}),
    Row('nseq129', pieces(12900, [(9, 24)] * 129), (1, -1), {1: 1513, -1: 1513},
        {'seq/ns/129': 1}),
    Row('bits57', _bits57, (1,), {1: 162137},
        {'lit/sampled/raw': 1, 'seq/bits/>=57': 1, 'block/repcodes-unconfirmed': 1}),
    Row('binary_m2', _binary_chunk, (1,), {1: 7676},
        {'norm/m2/spread': 1, 'seqtab/norm/m2': 1}),
    Row('text128k', lambda: L.datagen("text", BLOCK, 7), (1, 2, -1, -5), {1: 45091, 2: 43478, -1: 60526, -5: 69272},
        {'seqtab/norm/low/-1': 14, 'seq/LL/tablelog/9': 1, 'seq/ML/tablelog/9': 1}),
    Row('json40000', lambda: L.datagen("json", 40000, 7), (1,), {1: 8976},
        {'huf/limit/repay/no-symbol-at-rank': 1, 'huf/limit/overpaid': 1, 'huf/limit/overpaid/rank1-empty': 1}),
    Row('random128k', lambda: _rng(8).integers(0, 256, BLOCK, dtype=np.uint8), (1,), {1: 131084},
        {'lit/sampled/raw': 1}),
    Row('text4000', lambda: L.datagen("text", 4000, 7), (1,), {1: 1778},
        {'huf/maxnb/10': 1}),
    Row('text12000', lambda: L.datagen("text", 12000, 7), (1,), {1: 4676},
        {'seq/LL/tablelog/7': 1}),
    Row('text24000', lambda: L.datagen("text", 24000, 7), (1,), {1: 9000},
        {'seq/LL/tablelog/8': 1}),
    Row('ratio19', pieces(19, [(6, 24)] * 10), (1,), {1: 231},
        {'lit/suspect/ratio=19': 1, 'seq/OF/type/predef-by-count': 1}),
    Row('ratio20', pieces(20, [(7, 24)] * 10), (1,), {1: 241},
        {'lit/suspect/ratio=20': 1, 'huf/maxnb/8': 1}),
    Row('uniform3000', lambda: _rng(9).integers(0, 256, 3000, dtype=np.uint8), (1,), {1: 3010},
        {'lit/flat/raw': 1}),
    Row('ml_flat', periodic(0, shuffled(0, _FLAT_ML)), (1, -1), {1: 906, -1: 906},
        {'seq/ML/type/predef-by-flatness': 1, 'seq/LL/type/rle': 1},
        at={-1: {'seq/ML/type/predef-by-flatness': 1}}),
    Row('m2_second_pass', periodic(0, shuffled(0, _M2_ML)), (1,), {1: 2886},
        {'norm/m2/second-pass': 1, 'norm/m2/spread': 1, 'seqtab/norm/m2': 1, 'seq/ML/tablelog/6': 1}),
    edge_row('binary1m', 1,
             {'lit/sampled/passed': 8, 'hufw/ncount/flush-mid-run': 3}),
    edge_row('rle_literals', 1,
             {'lit/rle': 1}),
    edge_row('sparse1200', 1,
             {'huf/maxnb/6': 1, 'seq/LL/tablelog/5': 1}),
    dfast_row('runs40000', 491,
              {'huf/weights/rle': 1}),
    edge_row('tail_repeat', 1,
             {'seq/ll>=65536': 1}),
    dfast_row('text5', 14,
              {'block/len<7': 1}),
    edge_row('zeros300k', 1,
             {'block/rle': 1, 'block/rle-refused-first-block': 2}),
    edge_row('sparse300', 1,
             {'seq/OF/type/rle': 2, 'seq/ML/type/rle': 1}),
]
