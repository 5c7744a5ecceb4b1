"""tests/zstd_entropy_census.py -- which decisions of zstd's entropy stage an input causes.  No GPU; the entropy-side
counterpart of tests/lzc_census.py and tests/zstd_dfast_census.py.

walk(data, level) compresses one chunk with the restatement (oracle/zstd1_oracle.c; its bytes are the reference
build's, tests/test_zstd_oracle.py) and returns (frame, Counter of the classes below).  The counters live in the
restatement's own functions (oracle_zstd_compress_census: one body with oracle_zstd_compress), so a class is an event
of the reference algorithm on that input -- nothing here models lanes or waves.  Reference lines are zstd 1.5.2's,
under lib/compress/ (huf: huf_compress.c, lit: zstd_compress_literals.c, fse: fse_compress.c, seq:
zstd_compress_sequences.c, zc: zstd_compress.c; a few lines either way); the kernel side is namespace ze of
lzbench_amd/csrc/zstdc.h and zstdc_entropy_body.inc ("body").

DOC below holds, for every class, the reference line and the kernel function or branch it drives; UNREACHABLE and
NOT_REACHED hold the argument or the search of each class no named input reaches.  The module's docstring is
rendered from them, so the table, the class list and the two sets cannot drift apart
(tests/test_zstd_entropy_census.py compares them exactly).  "*/" stands for the two FSE call sites, seqtab/ (the three
sequence tables, ze::encode_sequences' lane-0 loop) and hufw/ (the Huffman weights, ze::huf_compress_weights);
"seq/T/" for the three tables seq/LL/, seq/OF/, seq/ML/.

Against the issue's starting list.  Added: lit/stream>65535, huf/maxnb/by-max11 and by-floor5 (the other two terms),
ncount/zero-run/0, block/repcodes-confirmed.  Changed: the FSE events are kept per call site (seqtab, hufw), not per
sequence table: the restatement and the kernel have two call sites, the three tables share one loop, and which
table took which path shows in seq/T/type and seq/T/tablelog; the exits of FSE_normalizeM2 are counted once for
both sites.  lit/raw/streams-too-large is two classes (old and new table).  Dropped: lit/table/unrepresentable (the
same event as huf/table/maxs>128-direct-refused); block/skipped-by-parser (for the calls the restatement covers it
is block/len<7: the match kernels set word 32 for blocks under 7 bytes; the dictionary variants also set it for a
chunk without a table, which is no event of the reference)."""

CL, ES = "ze::compress_literals", "ze::encode_sequences"
# normalised class -> (reference, kernel function or branch)
DOC = {
    "lit/gate/n<=63": ("lit:97-98 srcSize <= minLitSize", CL + " `P.lit_off || n <= 63`: ze::lit_raw"),
    "lit/gate/n=63": ("lit:98, the last size stored raw", CL + " the same test, true"),
    "lit/gate/n=64": ("lit:98, the first size past the gate", CL + " the same test, false"),
    "lit/off": ("lit:89 ZSTD_literalsCompressionIsDisabled (negative levels)", CL + " `P.lit_off`"),
    "lit/sampled/raw": ("huf:1212-1221 suspectUncompressible, n >= 40960", CL + " `b1 + b2 <= 68`: ze::lit_raw"),
    "lit/sampled/passed": ("huf:1221", CL + " the two histo256 / histo_stats of 4096 bytes, then on"),
    "lit/suspect/ratio=19": ("zc:2607 literals / sequences under 20", CL + " `suspect` false"),
    "lit/suspect/ratio=20": ("zc:2607 at 20", CL + " `suspect` true"),
    "lit/rle": ("huf:1227 largest == srcSize", CL + " `largest == n`: the RLE header, lane 0"),
    "lit/flat/raw": ("huf:1228 largest <= (n >> 7) + 4", CL + " the same test: ze::lit_raw"),
    "lit/repeat/invalid": ("huf:1233-1235 HUF_validateCTable fails", CL + " the ballot over L.cnt / L.pnb"),
    "lit/repeat/small-direct": ("huf:1238 preferRepeat", CL + " `n <= 1024 && repeat`: huf_streams with L.pnb"),
    "lit/repeat/old-by-estimate": ("huf:1266 oldSize <= hSize + newSize", CL + " `useOld`, first term"),
    "lit/repeat/old-by-h+12": ("huf:1266 hSize + 12 >= srcSize", CL + " `useOld`, second term"),
    "lit/repeat/new-table": ("huf:1263-1270 neither", CL + " `useOld` false with `repeat`"),
    "lit/raw/h+12>=n": ("huf:1273", CL + " `h + 12 >= n`: ze::lit_raw"),
    "lit/raw/streams-too-large/old": ("huf:1135-1147 with the old table", CL + " `c == 0 || c >= n - 1`; "
                                      "ze::huf_streams' early `tot >= n - 1`"),
    "lit/raw/streams-too-large/new": ("huf:1135-1147 with the new table", CL + " `c2 == 0 || h + c2 >= n - 1`; "
                                      "ze::huf_streams' early return"),
    "lit/raw/mingain": ("lit:121 cLitSize >= srcSize - minGain", CL + " `c >= n - minGain`"),
    "lit/hdr/3": ("lit:80 lhSize, n < 1024", CL + " `lh == 3` header store"),
    "lit/hdr/4": ("lit:80, n < 16384", CL + " `lh == 4`"),
    "lit/hdr/5": ("lit:80, n >= 16384", CL + " `lh == 5`: the fifth byte"),
    "lit/streams/1": ("lit:82 singleStream, n < 256", "ze::huf_streams `four` 0"),
    "lit/streams/4": ("lit:82", "ze::huf_streams `four` 1: the jump table"),
    "lit/stream>65535": ("huf:1100-1125 cSize > 65535", "ze::huf_streams `sizes[sidx] > 65535`"),
    **{f"huf/maxnb/{k}": ("fse:365-377 the log HUF_optimalTableLog picks", f"ze::fse_opt_log(11, ..) = {k}, into "
                          "ze::huf_build") for k in range(5, 12)},
    "huf/maxnb/by-max11": ("fse:369 maxTableLog", "ze::fse_opt_log `tl = maxLog`"),
    "huf/maxnb/by-srcsize": ("fse:371 maxBitsSrc", "ze::fse_opt_log `srcBits < tl`"),
    "huf/maxnb/by-minbits": ("fse:372 minBits", "ze::fse_opt_log `mb > tl`"),
    "huf/maxnb/by-floor5": ("fse:373 FSE_MIN_TABLELOG", "ze::fse_opt_log `tl < 5`"),
    "huf/limit/not-needed": ("huf:312", "ze::huf_limit `largest <= maxNb`"),
    "huf/limit/fired": ("huf:314-", "ze::huf_limit past it: the cost loop"),
    "huf/limit/repay/dec>1": ("huf:358-371", "ze::huf_limit's `for (; dec > 1; dec--)` leaves dec > 1"),
    "huf/limit/repay/no-symbol-at-rank": ("huf:373-374", "ze::huf_limit `while (rankLast[dec] == NONE) dec++`"),
    "huf/limit/overpaid": ("huf:408", "ze::huf_limit `while (cost < 0)`"),
    "huf/limit/overpaid/rank1-empty": ("huf:412", "ze::huf_limit `rankLast[1] == NONE`"),
    "huf/sort/bucket>=165": ("huf:585-592 bucketSize > 1", "ze::huf_build's bucket loop: ze::huf_qsort"),
    "huf/sort/qsort-partitioned": ("huf:528 over 8 elements", "ze::huf_qsort / huf_partition, task stack L.qs"),
    "huf/weights/wn<=1": ("huf:105", "ze::huf_compress_weights `wn <= 1`"),
    "huf/weights/rle": ("huf:109", "ze::huf_compress_weights `big == wn`"),
    "huf/weights/all-distinct": ("huf:110", "ze::huf_compress_weights `big == 1`"),
    "huf/weights/fse": ("huf:112-129", "ze::huf_compress_weights: normalize, write, build, encode"),
    "huf/weights/fse-too-large": ("huf:195 hSize >= maxSymbolValue / 2", "ze::huf_write_table falls to the nibbles"),
    "huf/weights/odd-count": ("fse:611 srcSize & 1", "ze::huf_compress_weights `wn & 1`"),
    "huf/table/direct": ("huf:199-207", "ze::huf_write_table's nibble loop"),
    "huf/table/fse": ("huf:195-197", "ze::huf_write_table `h > 1 && h < maxs / 2`"),
    "huf/table/maxs>128-direct-refused": ("huf:199 maxSymbolValue > 128", "ze::huf_write_table -1; " + CL +
                                          " `h < 0`: ze::lit_raw"),
    "*/norm/fast": ("fse:516", "ze::fse_normalize `norm[largest] += still`"),
    "*/norm/p<8-rounded-up": ("fse:502-506 rtbTable", "ze::fse_normalize `p < 8` correction"),
    "*/norm/low/-1": ("fse:497 with useLowProbCount (n1 >= 2048)", "ze::fse_normalize `cnt[s] <= lowThreshold`, "
                      "low -1; fse_build's high-threshold placement"),
    "*/norm/low/+1": ("fse:497 without", "ze::fse_normalize the same test, low 1"),
    "*/norm/m2": ("fse:510", "ze::fse_normalize calls ze::fse_norm_m2"),
    "norm/m2/todist=0": ("fse:420", "ze::fse_norm_m2 `toDist == 0`"),
    "norm/m2/second-pass": ("fse:423", "ze::fse_norm_m2 `(total / toDist) > lowOne`"),
    "norm/m2/all-low": ("fse:436", "ze::fse_norm_m2 `distributed == maxs + 1`"),
    "norm/m2/total=0": ("fse:447", "ze::fse_norm_m2 `total == 0`"),
    "norm/m2/spread": ("fse:457-471", "ze::fse_norm_m2's rstep loop"),
    "*/ncount/zero-run/0": ("fse:261-280 no further zero", "ze::fse_write_ncount `prev0`: one 2-bit field of 0"),
    "*/ncount/zero-run/1-2": ("fse:276", "ze::fse_write_ncount one 2-bit field of 1 or 2"),
    "*/ncount/zero-run/3+": ("fse:272-275", "ze::fse_write_ncount `while (sym >= start + 3)`"),
    "*/ncount/zero-run/24+": ("fse:264-271", "ze::fse_write_ncount `while (sym >= start + 24)`: 0xFFFF"),
    "*/ncount/count>=threshold": ("fse:291", "ze::fse_write_ncount `c >= threshold`"),
    "*/ncount/ends-early": ("fse:259 remaining <= 1", "ze::fse_write_ncount's loop condition"),
    "*/ncount/flush-mid-run": ("fse:279", "ze::fse_write_ncount `nb > 16` inside `prev0`"),
    "seq/T/type/rle": ("seq:166-176 mostFrequent == nbSeq", ES + " `big == ns`: ze::fse_build_rle"),
    "seq/T/type/rle-as-predef": ("seq:169 nbSeq <= 2", ES + " `defOk && ns <= 2`"),
    "seq/T/type/predef-by-count": ("seq:192 nbSeq < dynamicFse_nbSeq_min", ES + " `ns < dynMin` (LZH_ZSTD_STRATEGY)"),
    "seq/T/type/predef-by-flatness": ("seq:193", ES + " `big < ns >> (defLog - 1)`"),
    "seq/T/type/fse": ("seq:197-", ES + " `ty == 2`: normalize, write, build"),
    "seq/T/type/default-refused": ("zc:2506 the offset table's max > DefaultMaxOff", ES + " `defOk` 0"),
    "seq/T/last-count-trick/taken": ("seq:271 count[last code] > 1", ES + " `cnt[cl[t]] > 1`"),
    "seq/T/last-count-trick/not": ("seq:271", ES + " the same test, false"),
    **{f"seq/T/tablelog/{k}": ("seq:269 FSE_optimalTableLog", f"ze::fse_opt_log(fseLog[t], ..) = {k}: the size of "
                               "L.fse[t].st in use") for k in range(5, 10)},
    **{f"seq/ns%64/{k}": ("no branch of the reference", ES + f" the last round's gn = {k or 64}: "
                          + ("no remainder round" if k == 0 else
                             f"{'the unrolled 4-step chain once and ' if k >= 4 else ''}the remainder loop"))
       for k in range(6)},
    "seq/ns/1": ("seq:290-382 only the first symbol's FSE_initCState2", ES + " one round, the init alone"),
    "seq/ns/63": ("-", ES + " one round short of full"),
    "seq/ns/64": ("-", ES + " one full round with the init: 15 unrolled steps and 3"),
    "seq/ns/65": ("-", ES + " a full round and a round of 1"),
    "seq/ns/128": ("-", ES + " two full rounds, the second without init: 16 unrolled steps"),
    "seq/ns/129": ("-", ES + " three rounds"),
    "seq/bits/>=32": ("no branch of the reference", ES + " put(): a field crosses a dword of L.stage"),
    "seq/bits/>=57": ("no branch of the reference", ES + " put(): one sequence over two dwords of the window"),
    "seq/ll>=65536": ("LL code 35, 16 extra bits", "ze::ll_code / ll_bits `hb32(ll)`"),
    "seq/ml>=65539": ("ML code 52, 16 extra bits", "ze::ml_code / ml_bits `hb32(mb)`"),
    "seq/ofcode>=17": ("offsets of 128 KiB and more", ES + " `nof = ofc` of 17 and more bits in put()"),
    "block/len<7": ("zc:2821", "body `skip` (word 32 of the frame's scratch, set by the match kernel)"),
    "block/raw/mingain": ("zc:2704 ZSTD_minGain", "body `csize >= len - ((len >> 6) + 2)`"),
    "block/raw/sequences-failed": ("zc:2666", ES + " `lastCount + bs < 4`: 0"),
    "block/rle": ("zc:3795 ZSTD_isRLE", "body `k > 0 && csize < 25` and the ballot"),
    "block/rle-refused-first-block": ("zc:3793 !frame->isFirstBlock", "body `k > 0` false"),
    "block/cmp/new-huf-table-kept": ("zc:3813 confirm", "body `newTable`: the store to zc::kHufOff"),
    "block/repcodes-confirmed": ("zc:3813", "body: words 16 / 20 from 8 / 12"),
    "block/repcodes-unconfirmed": ("zc:3813 not reached", "body: words 16 / 20 keep the older block's"),
}
from collections import Counter

import numpy as np

import oracle_lib as O

# in the order of oracle.h's ORACLE_ZSE_*
_BASE = (
    "lit/gate/n<=63", "lit/gate/n=63", "lit/gate/n=64", "lit/off", "lit/sampled/raw", "lit/sampled/passed",
    "lit/suspect/ratio=19", "lit/suspect/ratio=20", "lit/rle", "lit/flat/raw", "lit/repeat/invalid",
    "lit/repeat/small-direct", "lit/repeat/old-by-estimate", "lit/repeat/old-by-h+12", "lit/repeat/new-table",
    "lit/raw/h+12>=n", "lit/raw/streams-too-large/old", "lit/raw/streams-too-large/new", "lit/raw/mingain",
    "lit/hdr/3", "lit/hdr/4", "lit/hdr/5", "lit/streams/1", "lit/streams/4", "lit/stream>65535",
    "huf/maxnb/5", "huf/maxnb/6", "huf/maxnb/7", "huf/maxnb/8", "huf/maxnb/9", "huf/maxnb/10", "huf/maxnb/11",
    "huf/maxnb/by-max11", "huf/maxnb/by-srcsize", "huf/maxnb/by-minbits", "huf/maxnb/by-floor5",
    "huf/limit/not-needed", "huf/limit/fired", "huf/limit/repay/dec>1", "huf/limit/repay/no-symbol-at-rank",
    "huf/limit/overpaid", "huf/limit/overpaid/rank1-empty", "huf/sort/bucket>=165", "huf/sort/qsort-partitioned",
    "huf/weights/wn<=1", "huf/weights/rle", "huf/weights/all-distinct", "huf/weights/fse",
    "huf/weights/fse-too-large", "huf/weights/odd-count", "huf/table/direct", "huf/table/fse",
    "huf/table/maxs>128-direct-refused",
    "norm/m2/todist=0", "norm/m2/second-pass", "norm/m2/all-low", "norm/m2/total=0", "norm/m2/spread",
    "seq/ns%64/0", "seq/ns%64/1", "seq/ns%64/2", "seq/ns%64/3", "seq/ns%64/4", "seq/ns%64/5",
    "seq/ns/1", "seq/ns/63", "seq/ns/64", "seq/ns/65", "seq/ns/128", "seq/ns/129",
    "seq/bits/>=32", "seq/bits/>=57", "seq/ll>=65536", "seq/ml>=65539", "seq/ofcode>=17",
    "block/len<7", "block/raw/mingain", "block/raw/sequences-failed", "block/rle", "block/rle-refused-first-block",
    "block/cmp/new-huf-table-kept", "block/repcodes-confirmed", "block/repcodes-unconfirmed")
_FSE = ("norm/fast", "norm/p<8-rounded-up", "norm/low/-1", "norm/low/+1", "norm/m2", "ncount/zero-run/0",
        "ncount/zero-run/1-2", "ncount/zero-run/3+", "ncount/zero-run/24+", "ncount/count>=threshold",
        "ncount/ends-early", "ncount/flush-mid-run")
_TAB = ("type/rle", "type/rle-as-predef", "type/predef-by-count", "type/predef-by-flatness", "type/fse",
        "type/default-refused", "last-count-trick/taken", "last-count-trick/not", "tablelog/5", "tablelog/6",
        "tablelog/7", "tablelog/8", "tablelog/9")
SITES = ("seqtab", "hufw")
TABLES = ("LL", "OF", "ML")
ALL_CLASSES = (list(_BASE) + [f"{s}/{n}" for s in SITES for n in _FSE]
               + [f"seq/{t}/{n}" for t in TABLES for n in _TAB])
assert len(set(ALL_CLASSES)) == len(ALL_CLASSES)

# class -> the argument from the reference; the tests fail if one turns up on any input or corpus
UNREACHABLE = {
    "lit/repeat/old-by-h+12": "a valid kept table and n <= 1024 is small-direct, and h <= 129 < 1025 - 12",
    "lit/stream>65535": "a stream holds at most 32768 literals of at most 11 bits",
    "norm/m2/todist=0": "the table log is at least hb(maxs) + 2 (sequences: hb(n) + 1 is no smaller from 72 sequences "
                        "on; weights: the floor of 5 against 13 symbols), so at most half the slots have a symbol",
    "norm/m2/all-low": "all symbols low in the first pass needs 2/3 of the slots; in the second, toDist <= 1.5 R with "
                       "toDist = 2^tl - L and R + L <= 2^(tl - 1): impossible",
    "norm/m2/total=0": "all-low with a gap in the alphabet: the same bound",
    "seqtab/ncount/ends-early": "the counts sum to the table size and maxs, the last symbol, has a count",
    "hufw/ncount/ends-early": "as for seqtab",
    "hufw/norm/low/-1": "HUF_compressWeights passes useLowProbCount 0",
    "hufw/ncount/zero-run/24+": "13 weights",
    "seq/LL/type/default-refused": "the literal-length default is always allowed",
    "seq/OF/type/default-refused": "an offset code above 28 needs a 512 MiB window and chunks end at 16 MiB",
    "seq/ML/type/default-refused": "the match-length default is always allowed",
    "seq/OF/tablelog/9": "OffFSELog is 8 and the minimum for 32 codes is 6",
    "seq/LL/type/predef-by-flatness": "needs mostFrequent < ns / 32, so at least 33 literal-length codes with ns >= "
                                      "32 (mostFrequent + 1): from mostFrequent 8 up, and eight runs each of the 33 "
                                      "cheapest codes are 133504 literals, more than a block",
}
# class -> the search that was tried and its bound
NOT_REACHED = {
    "huf/table/maxs>128-direct-refused":
        "needs over 128 symbols whose weights FSE cannot bring under maxs / 2 bytes.  400 blocks of 300 - 6000 "
        "literals "
        "over 129 - 256 symbols with geometric weights raised to a power of 0.5 - 3: none",
    "lit/raw/h+12>=n":
        "needs a table description of 52 bytes for 64 .. 77 literals.  400 literals() inputs of that size over 57 .. "
        "72 "
        "distinct symbols up to 127: the weights always compressed (huf/table/fse) and every section ended at "
        "lit/raw/streams-too-large/new",
    "block/raw/sequences-failed":
        "needs 72 sequences in under two bytes of stream: LL and OF tables RLE and an ML table whose minority code is "
        "the last sequence's only.  periodic() with 71 .. 200 matches of 8 bytes and a last one of 9 or 12 (260 "
        "inputs): "
        "LL is RLE, but the first match is found by its hash and the others by the repeat offset, so OF has two codes "
        "and a table of its own; 71 codes of probability 31 / 32 alone cost about 3.3 bits",
    "hufw/norm/m2":
        "400 separators() inputs of 200 - 1300 literals drawn from 20 - 250 symbols with geometric weights raised to a "
        "power of 1 - 3: none; the 32 slots against at most 13 weights, few of them rare by Kraft's sum, leave the "
        "fast "
        "path little to overshoot",
    "seq/OF/type/predef-by-flatness":
        "needs each of 17 and more offset codes, repcodes included, 4 times and more in one block.  The 256 chunks of "
        "64 KiB of 4 MiB each of datagen binary, mixed, json and text (seed 77): none",
}


def _expand(k):
    if k.startswith("*/"):
        return [f"{s}/{k[2:]}" for s in SITES]
    if k.startswith("seq/T/"):
        return [f"seq/{t}/{k[6:]}" for t in TABLES]
    return [k]


def documented():
    """the classes DOC documents, expanded"""
    return [c for k in DOC for c in _expand(k)]


def _check_sets():
    assert sorted(documented()) == sorted(ALL_CLASSES), set(documented()) ^ set(ALL_CLASSES)
    assert set(UNREACHABLE) <= set(ALL_CLASSES) and set(NOT_REACHED) <= set(ALL_CLASSES)
    assert not set(UNREACHABLE) & set(NOT_REACHED)


def _render():
    import textwrap
    def block(title, d, fmt):
        out = [title]
        for k, v in d.items():
            out += textwrap.wrap(fmt(k, v), 116, initial_indent="  ", subsequent_indent="      ")
        return "\n".join(out)
    return "\n\n".join([
        block("Classes (reference; kernel):", DOC, lambda k, v: f"{k}   {v[0]}; {v[1]}"),
        block("UNREACHABLE (argued from the reference; the tests fail if one turns up):", UNREACHABLE,
              lambda k, v: f"{k}   {v}"),
        block("NOT_REACHED (the search tried and its bound):", NOT_REACHED, lambda k, v: f"{k}   {v}")])


_check_sets()
__doc__ += "\n\n" + _render()


def walk(data, level=1):
    """(frame, Counter of classes) of one chunk at that level: the restatement's frame (no raw-store rule)"""
    frame, c = O.zstd_compress_census(np.ascontiguousarray(data, dtype=np.uint8), level)
    assert not c[len(ALL_CLASSES):].any(), "the restatement counts an event this file does not name"
    return frame, Counter({n: int(v) for n, v in zip(ALL_CLASSES, c) if v})


def walk_chunks(data, chunk, level=1):
    """the Counter of a buffer compressed as chunks of `chunk` bytes (lzbench's loop)"""
    u = Counter()
    for a in range(0, max(len(data), 1), chunk):
        u.update(walk(data[a: a + chunk], level)[1])
    return u
