"""tests/zstd_dfast_census.py -- which events of zstd's level-3 (double-fast) parser an input causes.  No GPU; the
level-3 counterpart of tests/lzc_census.py.

walk(data) runs oracle/zstd_dfast_census.cpp (oracle/libzdfcensus.so): zdf::dfast_block of
lzbench_amd/csrc/zstd_dfast_parse.h -- the template the match kernel runs -- over a host environment, frame-wise as
zstdc_dfast_match_body.inc does.  The counters live in that environment and in the wrapper around each block; the
header is untouched.  Because the walk is shared with the kernel it is anchored to the reference and not to itself by
tests/test_zstd_dfast_census.py (block by block against the reference build's frame, sequence by sequence against
ZSTD_generateSequences).  Lines are zstd 1.5.2's lib/compress/zstd_double_fast.c unless another file is named; the
kernel side is lzbench_amd/csrc/zstdc_dfast.h (WaveEnv) with count_fwd / count_bwd / lit_copy / GlbTab of
zstdc.h.

  params/row/n>262144, n<=262144, n<=131072, n<=16384   the clevels.h row of level 3 (table sizes, mls)
  params/mls4, mls5            minMatch of the row: hash_short over 4 or 5 bytes
  params/wlog-clamped          zstd_compress.c ZSTD_adjustCParams_internal: windowLog cut to the source's log
  params/hlog-clamped, clog-clamped   hashLog cut to windowLog + 1, chainLog to windowLog (the tables' sizes)
  params/wlog-raised-to-10     ZSTD_WINDOWLOG_ABSOLUTEMIN (frames up to 512 bytes)
  frame/blocks/1, 2, 3+        launches of the kernel pair per frame; tables and repcodes carried
  block/first, later           :108 ip += (ip == prefixLowest)
  block/under-7-bytes          zstd_compress.c:2821, no search at all (the body's `be - bs < 7`)
  block/too-short-to-search    :113 ip1 > ilimit on the first pass
  block/dl>0, plow>dl          the window has slid before / inside the block (:65 ZSTD_getLowestPrefixIndex)
  block/off2-saved, off1-saved :103, :104; block/saved-restored: :179-180 the saved offset returned
  block/rep-saved-on-later-block  the same on a block that is not the frame's first (see UNREACHABLE)
  block/repcodes-unconfirmed   the block before was stored raw or as RLE: zstd_compress.c:3813 keeps the old repcodes
                               (hdr words 16/20 of the frame's scratch are not overwritten by the entropy kernel)
  search/rep-hit               :128-135 repcode at ip + 1
  search/long-hit              :140-146 long match at ip
  search/short-kept            :153-156, :199 the short match, no long one at ip + 1
  search/long-at-ip+1          :188-194 _search_next_long takes the long match at ip1
  search/ran-out, ends-at-match   :171 the loop ends in the search / :113 after a match
  step/1, 2, 3, 4+             ip1 - ip at a found match (:160-164, every 256 bytes searched without one)
  post/hl1-inserted, hl1-skipped   :209-217 the complementary long-table insertion, skipped at a step of 4 or more
  reject/{long,short}/empty    a table entry of 0
  reject/{long,short}/stale    a non-zero index at or below prefixLowestIndex (:140, :153, :188)
  reject/{long,short}/collision   an index in range whose bytes differ
  hit/fresh-long, fresh-short  a match from an entry stored just before the last fence (by the previous searched
                               position or the previous match's insertions): store, s_waitcnt, load (GlbTab::fence)
  catchup/0, 1-63, 64, 65+     :145/:193/:201; zc::count_bwd answers 64 bytes a round, so 64 and more take a second
  catchup/to-anchor, to-plow   which of the two conditions ended it
  count/0, 1-255, 256, 257-511, 512+   ZSTD_count past the seed; zc::count_fwd answers 256 bytes a round
  count/to-block-end           the count ran into iend
  ml/>=65539, ml/>=65539-rep   the match-length long-length escape (ZSTD_storeSeq), for found and repcode matches
  lit/0, 1-63, 64, 65-255, 256, >256   literal run of a sequence: zc::lit_copy's byte-per-lane, dword and copy_span paths
  lit/>=65536                  the literal-length escape
  off/1, off/2-7               offsets under 8: source and target of the 8-byte compare overlap
  off/>=65536, off/earlier-block   the match source lies 64 KiB back / before the block's start
  off/window                   an offset equal to the window size (see UNREACHABLE)
  post/insert-done, insert-skipped   :227 ip <= ilimit after the match
  imm-rep/0, 1, 2+             :238 rounds of the immediate-repcode loop after a match; imm-rep/ends-block: its match
                               passes ilimit
  block/no-sequences, block/tail/0   what the block hands the entropy stage
  nseq/31, 32, 33, 36, 37, 63, 64, 65, 72, 73   sequences of a block around ZSTD_selectEncodingType's thresholds
                               (zstd_compress_sequences.c:182-192: 32 for OF and 64 for LL/ML at strategy 2, 36 and
                               72 at strategy 1): LZH_ZSTD_STRATEGY 2 of the level-3 entropy kernel
  invariant/negative-read      a read below the frame's first byte (WaveEnv's max(pos, 0) clamps)
  invariant/read-past-frame, load-before-fence, model-mismatch   must be 0: a read past n, a table load of a slot
                               stored since the last fence, a walk the environment's state machine did not expect
  sequences                    every stored sequence

Against the issue's starting list: added block/under-7-bytes, block/repcodes-unconfirmed, search/ends-at-match,
step/1, count/to-block-end (instead of "a match ending at the block end": the same event), catchup/64 as a class of
its own (exactly one full round) and the four invariant counters.  The rejections of idxl1 in _search_next_long
count as reject/long.  Dropped: nothing.

UNREACHABLE (argued from the reference; the test fails if one turns up):
  block/off1-saved             offset_1 > maxRep needs a first repcode above current - windowLow.  On the first block
                               current = 1 and rep[0] = 1 (repStartValue); on later blocks see the next entry.
  block/rep-saved-on-later-block   on block k > 0, current = k * blockSize >= maxRep's window; every earlier offset is
                               below the position it was found at, so below current, and within the window (below);
                               the start values 1 and 4 are below any block size.
  off/window                   a match source index exceeds prefixLowestIndex = blockEnd - windowSize once the window
                               is full, and ip <= blockEnd - 8, so an offset is at most windowSize - 9; a repcode is
                               an earlier offset.
  invariant/*                  by construction of the walk.
"""
import ctypes as C
import os
from collections import Counter

import numpy as np

import oracle_lib as O

LIB_PATH = os.path.join(O.ROOT, "oracle", "libzdfcensus.so")
_lib = None

INVARIANTS = ("invariant/negative-read", "invariant/read-past-frame", "invariant/load-before-fence",
              "invariant/model-mismatch")
UNREACHABLE = ("block/off1-saved", "block/rep-saved-on-later-block", "off/window") + INVARIANTS


def have_lib() -> bool:
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        L.zdf_census_nclasses.restype = C.c_int
        L.zdf_census_class_name.restype = C.c_char_p
        L.zdf_census_class_name.argtypes = [C.c_int]
        L.zdf_census_frame.restype = C.c_int64
        L.zdf_census_frame.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                       C.c_uint64, C.c_void_p]
        _lib = L
    return _lib


def classes():
    """the class names, in the library's order"""
    L = lib()
    return [L.zdf_census_class_name(i).decode() for i in range(L.zdf_census_nclasses())]


def documented():
    """the class names the table above lists (its first column, expanded)"""
    return ["params/row/n>262144", "params/row/n<=262144", "params/row/n<=131072", "params/row/n<=16384",
            "params/mls4", "params/mls5", "params/wlog-clamped", "params/hlog-clamped", "params/clog-clamped",
            "params/wlog-raised-to-10", "frame/blocks/1", "frame/blocks/2", "frame/blocks/3+", "block/first",
            "block/later", "block/under-7-bytes", "block/too-short-to-search", "block/dl>0", "block/plow>dl",
            "block/off1-saved", "block/off2-saved", "block/rep-saved-on-later-block", "block/saved-restored",
            "block/repcodes-unconfirmed", "search/rep-hit", "search/long-hit", "search/short-kept",
            "search/long-at-ip+1", "search/ran-out", "search/ends-at-match", "step/1", "step/2", "step/3", "step/4+",
            "post/hl1-inserted", "post/hl1-skipped", "reject/long/empty", "reject/long/stale", "reject/long/collision",
            "reject/short/empty", "reject/short/stale", "reject/short/collision", "hit/fresh-long", "hit/fresh-short",
            "catchup/0", "catchup/1-63", "catchup/64", "catchup/65+", "catchup/to-anchor", "catchup/to-plow",
            "count/0", "count/1-255", "count/256", "count/257-511", "count/512+", "count/to-block-end", "ml/>=65539",
            "ml/>=65539-rep", "lit/0", "lit/1-63", "lit/64", "lit/65-255", "lit/256", "lit/>256", "lit/>=65536",
            "off/1", "off/2-7", "off/>=65536", "off/earlier-block", "off/window", "post/insert-done",
            "post/insert-skipped", "imm-rep/0", "imm-rep/1", "imm-rep/2+", "imm-rep/ends-block", "block/no-sequences",
            "block/tail/0"] + [f"nseq/{k}" for k in (31, 32, 33, 36, 37, 63, 64, 65, 72, 73)] + list(INVARIANTS) + [
            "sequences"]


def block_size(n: int) -> int:
    """the block size of a level-3 frame of n bytes: min(128 KiB, window size, n)"""
    wlog = (21, 18, 17, 14)[(n <= 262144) + (n <= 131072) + (n <= 16384)]
    wlog = max(min(wlog, max((n - 1).bit_length(), 6) if n >= 64 else 6), 10)
    return max(min(1 << wlog, 131072, n), 1)


def walk(data, confirm=None):
    """(Counter of classes, [(nseq, literal bytes, tail literals, searched) per block], sequences as an (N, 4) array
    of literal length, offBase, match length, resolved offset).  confirm: per block, False where the reference did
    not confirm the block's repcodes (block_types(frame) != "cmp"); None: every block confirms."""
    L = lib()
    d = np.ascontiguousarray(data, dtype=np.uint8)
    n = len(d)
    nb = max((n + block_size(n) - 1) // block_size(n), 1)
    seqs = np.zeros((n // 4 + 16, 4), np.uint32)
    blocks = np.zeros((nb, 4), np.uint32)
    c = np.zeros(L.zdf_census_nclasses(), np.uint64)
    cf = None if confirm is None else np.ascontiguousarray(confirm, dtype=np.uint8)
    assert cf is None or len(cf) == nb, (len(cf), nb)
    src = d if n else np.zeros(1, np.uint8)
    r = L.zdf_census_frame(src.ctypes.data, n, None if cf is None else cf.ctypes.data, seqs.ctypes.data, len(seqs),
                           blocks.ctypes.data, nb, c.ctypes.data)
    assert r == nb, (r, nb)
    total = int(blocks[:, 0].sum())
    return (Counter({name: int(v) for name, v in zip(classes(), c) if v}), [tuple(int(x) for x in b) for b in blocks],
            seqs[:total].copy())


def rebuild(data, blocks, seqs):
    """replays literals and copies block by block; returns the bytes (the caller compares them with the input) and
    asserts that every block ends on its boundary and every offset stays inside the window and the output so far"""
    d = np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    n = len(d)
    bsz = block_size(n)
    wlog = (21, 18, 17, 14)[(n <= 262144) + (n <= 131072) + (n <= 16384)]
    window = 1 << max(min(wlog, max((n - 1).bit_length(), 6) if n >= 64 else 6), 10)
    out = bytearray()
    pos = s = 0
    for k, (nseq, lits, tail, _) in enumerate(blocks):
        start = pos
        for ll, _, ml, off in seqs[s:s + nseq].tolist():
            out += d[pos:pos + ll]
            pos += ll
            assert 0 < off <= len(out) and off <= window, (k, off, len(out))
            if off >= ml:
                out += out[len(out) - off:len(out) - off + ml]
            else:
                for _ in range(ml):
                    out.append(out[-off])
            pos += ml
        s += nseq
        out += d[pos:pos + tail]
        pos += tail
        assert pos == min((k + 1) * bsz, n), (k, pos)
        assert lits == sum(int(x) for x in seqs[s - nseq:s, 0]) + tail and pos - start >= lits
    assert s == len(seqs)
    return bytes(out)


def block_types(frame: bytes):
    """the block types of a frame, in order: "raw", "rle" or "cmp" (RFC 8878 3.1.1.2)"""
    import zstd_census as ZC
    frame = bytes(frame)
    p, _, _ = ZC.frame_header(frame)
    types = []
    while True:
        bh = int.from_bytes(frame[p:p + 3], "little")
        t = (bh >> 1) & 3
        types.append(("raw", "rle", "cmp")[t])
        p += 3 + (1 if t == 1 else bh >> 3)
        if bh & 1:
            return types


def ref_frame(data) -> bytes:
    """the reference build's level-3 frame of data as one chunk (no raw-store rule: the frame itself)"""
    d = np.ascontiguousarray(data, dtype=np.uint8)
    n = len(d)
    dst = np.zeros(n + n // 6 + 16384, np.uint8)
    src = d if n else np.zeros(1, np.uint8)
    r = O.ref().ref_zstd_compress(src.ctypes.data, n, dst.ctypes.data, len(dst), 3)
    assert r > 0
    return dst[:r].tobytes()


def have_ref_sequences() -> bool:
    return O.have_ref() and hasattr(O.ref(), "ref_zstd_generate_sequences")


def ref_sequences(data):
    """ZSTD_generateSequences of the reference build at level 3: per block ([(literal length, match length, offset,
    rep)], last literals)"""
    R = O.ref()
    f = R.ref_zstd_generate_sequences
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
    d = np.ascontiguousarray(data, dtype=np.uint8)
    out = np.zeros((len(d) // 3 + 1024, 4), np.uint32)
    r = f(d.ctypes.data, len(d), 3, out.ctypes.data, len(out))
    assert r >= 0
    blocks, cur = [], []
    for off, ll, ml, rep in out[:r].tolist():
        if off == 0 and ml == 0:
            blocks.append((cur, ll))
            cur = []
        else:
            cur.append((ll, ml, off, rep))
    assert not cur
    return blocks
