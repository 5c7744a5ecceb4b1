"""tests/zstd_edge_inputs.py -- small named inputs that steer the zstd compressor into the branches of the frame
format the corpora reach only by chance, each with the classes (tests/zstd_census.py) its reference frames must
contain and the packed size measured from both the restatement and the reference build (zstd 1.5.2, lzbench's
zstd row).  tests/test_zstd_census.py holds every row to its declaration on the CPU; tests/test_gpu_zstd_census.py
runs the rows through the GPU compressor and decoders.

The long-length escapes are declared through sizes (`shape`), since the census reads no sequence: `zeros128k` is
one block with one sequence, so its match is 131072 - regen bytes long (65539 and more: ML code 52 with 16 extra
bits); `tail_repeat` is 70000 random bytes and then their first 61072 again, one sequence whose match of
131072 - 70000 bytes can only be the repeated tail, so all 70000 literals precede it (65536 and more: LL code 35).

`rle_literals` reaches the two classes the corpora never do.  Block 1 is 1215 random bytes (values 1..254) and
zeros: the fast match finder indexes nearly every position of so short a literal run.  Block 2 is 71 sixteen-byte
slices of those random bytes, taken 17 apart so that no two overlap, each behind one byte 0xFF, then 0xFF to the
block's end: every slice is found by its hash and extended back to the 0xFF before it, which matches nothing, so
the block's literals are 72 times 0xFF -- an RLE literals section (level 1; the negative levels store literals
raw).  Block 3 repeats block 2: one match of 131072 bytes found at the block's first byte, so the block has a
sequence and no literal at all (`lit/regen=0`), and a long match length with literal length 0.
Search bound: this was the first construction tried after the two the issue records (slices of an earlier block
joined by a separator over text and over random data, where the slices' starts are not indexed).

`rle_literals_long` gets the 20-bit RLE header the same way with one offset: block 1 is random bytes (1..254, stored
raw), block 2 the same bytes with 0xFF over every 17th and over the last 64.  The first match is found at the
block's second byte (the first 255 positions of a block are all indexed), every later one is the repeat offset
checked two bytes past the 0xFF, extended back by the one byte the finder allows: 7708 literals, all 0xFF.

This census reads frame headers only: it cannot see why a literals section is raw, whether the Huffman depth limiter
or the secondary normalisation ran, whether a kept table was reused by the 1024-byte shortcut or by the estimate, or
which remainder of the 64-sequence rounds a block has.  tests/zstd_entropy_census.py counts those decisions in the
restatement itself, and tests/zstd_entropy_inputs.py reaches them (importing rows of this file where they already do).

Not reached from the compressor:
  lit/rle/hdr1   unreachable by construction: ZSTD_compressLiterals stores 63 literals and fewer raw, and the
                 1-byte header holds sizes up to 31 (the decoder's branch: a hand-built frame,
                 tests/test_gpu_zstd_census.py)
Unreachable by construction (asserted absent over everything the census tests compress):
  {LL,OF,ML}/repeat   at the fast strategy ZSTD_selectEncodingType takes set_repeat only when the previous
                 table is FSE_repeat_valid, which only a dictionary sets
  nseq/long      a 128 KiB block at minimum match 5-7 cannot hold 0x7F00 sequences"""
from typing import Callable, Dict, NamedTuple, Optional

import numpy as np

import lzbench_amd as L
from zstd_census import long_literal_frames, long_match_frames

BLOCK = 131072


class Edge(NamedTuple):
    name: str
    make: Callable[[], np.ndarray]
    chunk: int
    levels: tuple
    packed: Dict[int, int]                  # level -> packed bytes (restatement == reference build)
    classes: Dict[str, int]                 # class -> least count, at every level
    classes_at: Dict[int, Dict[str, int]] = {}      # more, at one level
    exact: Dict[str, int] = {}              # class -> exact count, at every level
    shape: Optional[Callable] = None        # predicate over census_packed's per-frame list


def _sparse(step):
    def make():
        d = np.zeros(262144, np.uint8)
        d[::step] = 7
        return d
    return make


def _tail_repeat():
    r = np.random.default_rng(1).integers(0, 256, 70000, dtype=np.uint8)
    return np.concatenate([r, r[:61072]])


def _rle_literals(nseg=71, seglen=16):
    rng = np.random.default_rng(3)
    prefix = rng.integers(1, 255, 8 + nseg * (seglen + 1), dtype=np.uint8)
    b1 = np.zeros(BLOCK, np.uint8)
    b1[:len(prefix)] = prefix
    b2 = np.full(BLOCK, 0xFF, np.uint8)
    for i in range(nseg):
        a = 4 + i * (seglen + 1)
        b2[i * (seglen + 1) + 1: (i + 1) * (seglen + 1)] = prefix[a: a + seglen]
    return np.concatenate([b1, b2, b2])


def _rle_literals_long():
    b1 = np.random.default_rng(0).integers(1, 255, BLOCK, dtype=np.uint8)
    b2 = b1.copy()
    b2[::17] = 0xFF
    b2[-64:] = 0xFF
    return np.concatenate([b1, b2])


def _one_sequence_blocks(per):
    return all(nseq == 1 for _, blocks in per for _, nseq in blocks)


PREDEF3 = {"LL/predef": 1, "OF/predef": 1, "ML/predef": 1}

EDGES = [
    Edge("zeros300k", lambda: np.zeros(300000, np.uint8), 262144, (1, -1, -5), {1: 46, -1: 46, -5: 54},
         {"block/rle": 1, **PREDEF3}, exact={"block/cmp": 2, "LL/predef": 2, "OF/predef": 2, "ML/predef": 2},
         shape=_one_sequence_blocks),
    # (the second block's first sequence is the repeat offset 2 of the first block)
    Edge("ab300k", lambda: np.frombuffer(b"ab" * 150000, np.uint8).copy(), 262144, (1, -1, -5), {1: 54, -1: 54, -5: 66},
         PREDEF3, exact={"block/cmp": 3, "LL/predef": 3, "OF/predef": 3, "ML/predef": 3}, shape=_one_sequence_blocks),
    Edge("zeros128k", lambda: np.zeros(BLOCK, np.uint8), BLOCK, (1, 2, -5), {1: 22, 2: 22, -5: 26},
         {"blocks/1": 1, **PREDEF3}, shape=lambda per: len(per) == 1 and len(long_match_frames(per)) == 1),
    Edge("tail_repeat", _tail_repeat, BLOCK, (1, 2, -1, -5), {1: 70026, 2: 70026, -1: 70026, -5: 70026},
         {"lit/raw/hdr3": 1, "blocks/1": 1},
         shape=lambda per: len(long_literal_frames(per)) == 1 and per[0][1] == [(70000, 1)]),
    Edge("sparse300", _sparse(300), 262144, (1, -3), {1: 1167, -3: 3548}, {"LL/rle": 1, "ML/rle": 1, "OF/rle": 2},
         classes_at={1: {"hufhdr/direct": 1, "lit/treeless/sf1": 1, "lit/huf/sf1": 1}, -3: {"lit/raw/hdr2": 2}}),
    Edge("sparse1000", _sparse(1000), 262144, (1, -3), {1: 442, -3: 1144}, {"LL/rle": 1, "OF/rle": 2, "nseq/128-32511": 2},
         classes_at={1: {"hufhdr/direct": 1}}),
    # (fewer than 256 literals a block: one Huffman stream, and the second block reuses the first one's table)
    Edge("sparse1200", _sparse(1200), 262144, (1, -3), {1: 389, -3: 987}, {"LL/rle": 1, "OF/rle": 2, "nseq/1-127": 2},
         classes_at={1: {"hufhdr/direct": 1, "lit/huf/sf0": 1, "lit/treeless/sf0": 1}}),
    Edge("binary1m", lambda: L.datagen("binary", 1 << 20, 24), 524288, (1,), {1: 737749},
         {"nseq/0": 1, "OF/predef": 1, "OF/rle": 1, "lit/huf/sf3": 1, "hufhdr/fse": 1}),
    Edge("rle_literals", _rle_literals, 3 * BLOCK, (1, -1), {1: 1288, -1: 1359},
         {"lit/regen=0": 1, "LL/rle": 1, "blocks/2+": 1},
         classes_at={1: {"lit/rle/hdr2": 1}},
         shape=lambda per: per[0][1][1] == (72, 72) and per[0][1][2] == (0, 1)),
    Edge("rle_literals_long", _rle_literals_long, 2 * BLOCK, (1,), {1: 131127},
         {"lit/rle/hdr3": 1, "block/raw": 1, "LL/rle": 1, "nseq/128-32511": 1},
         shape=lambda per: per[0][1] == [(7708, 7708)]),
]

# the classes that are documented above instead of being required of the compressor-side tests
COMPRESSOR_NOT_REACHED = {"lit/rle/hdr1"}
COMPRESSOR_UNREACHABLE = {"LL/repeat", "OF/repeat", "ML/repeat", "nseq/long"}


def single_block_edges(level):
    """the inputs of 128 KiB and less that have `level` in their row"""
    return [e for e in EDGES if e.chunk <= BLOCK and level in e.levels]
