"""tests/lzc_census.py -- which events of the LZ4 and snappy COMPRESSORS' parsers an input causes.  No GPU; the
encoder-side counterpart of tests/lz_census.py (which reads streams) and tests/zstd_census.py.

lz4(data, acc) and snappy(data) compress one chunk with the restatement (oracle/lz4_oracle.c, snappy_oracle.c; the
bytes are the reference build's, tests/test_oracle.py) and return (compressed bytes, Counter of the classes below).
The counters live in the restatement's own parse loop (oracle_lz4_compress_census, oracle_snappy_compress_census:
one body with the plain entry points), so a class is an event of the reference parser on that input -- nothing here
models how a kernel groups positions into batches.  The kernels' own branches are named next to the event that
drives them.

  LZ4 (LZ4_compress_fast, lz4.c:851-1240)
    lz4/table/byU16, /byU32     the chunk is under / at least 65547 bytes (hash4 over u16, hash5 over u32 + far check)
    lz4/n<13                    fewer than 13 bytes: no search, all literals
    lz4/hit/search              a sequence found by the search loop (a catch-up follows)
    lz4/hit/retest              a sequence found by the re-test at a match end (no literals, no catch-up)
    lz4/retest-chain>=8         eight re-test hits in a row (sequences of 3 bytes: a run batch full of members)
    lz4/catchup/0, /1-3, /4, /5-64, />64   bytes the match was extended backwards (the kernels' candidate window
                                answers up to 4; then a lane-parallel loop of 64 bytes a step)
    lz4/catchup/to-anchor       a catch-up that stopped at the previous match end
    lz4/catchup/to-start        a catch-up that stopped at the chunk's first byte
    lz4/count/0, /1-19, /20, /21-275, />275   bytes matched past the 4-byte seed (the window answers up to 20, one
                                step of the slow count 256 more)
    lz4/count/>262164           past 1024 steps of the slow count (the kernels' former step cap)
    lz4/count/to-matchlimit     a match that ends at matchlimit (n - 5)
    lz4/lit/0, /1-14, /15, /16-255, /256+   literal run of a sequence; /15 = the length byte 0
    lz4/lit/270                 the length bytes 255, 0
    lz4/ml/15                   count 15: the length byte 0
    lz4/ml/15+255               count 270: the length bytes 255, 0
    lz4/off/1, /2-3, /65535     the offset (1: a byte run, every lane of a batch in one slot; 65535: the last in reach)
    lz4/far/rejected            (byU32) a candidate more than 65535 back, not compared
    lz4/far/65536               ... exactly one byte too far
    lz4/step>1                  acceleration 1: a probe after the 64th of a search (stride batches)
    lz4/step>acc                acceleration > 1: the same
    lz4/end/search-ran-out      the parse ends in the search (forwardIp past mflimit)
    lz4/end/match-at-mflimit    the parse ends at a match end at or past mflimit
    lz4/last-literals/5         exactly the 5 bytes no match may cover
    lz4/sequences               every sequence (the kernel's `sequences` counter must equal it)

  snappy (snappy::RawCompress, snappy.cc:510-681, :1043-1111)
    snappy/table/256 .. /16384  a fragment compressed with a table of that many entries
    snappy/frag<15              a fragment of fewer than 15 bytes: no search
    snappy/frags/1, /2, />=4    fragments of the chunk (64 KiB each)
    snappy/hit/search, /hit/retest   a copy found by the search / right after a copy
    snappy/probe>16             a probe past the 16 unrolled ones
    snappy/probe/off>63         a probe more than 63 bytes into its search (the kernels' search batches)
    snappy/search-ran-out       the fragment ends in the search
    snappy/end/copy             the fragment ends at a copy's end
    snappy/copy1                a COPY_1 tag
    snappy/copy2/len>=12        a COPY_2 tag because of its length
    snappy/copy2/off>=2048      a COPY_2 tag of under 12 bytes because of its offset
    snappy/copy/64, /65-67, /68, />=132   match lengths where EmitCopy changes shape (65-67: 60 + the rest)
    snappy/lit/1-60, /61-256, /257-65536   the literal length forms (tag, one, two length bytes)
    snappy/lit>256-before-copy  a literal run over 256 bytes that a copy follows (the emission kernel lays a
                                group with such a run out record by record)
    snappy/lit/remainder        the literal that ends a fragment"""
from collections import Counter

import oracle_lib as O

LZ4_NAMES = ("table/byU16", "table/byU32", "n<13", "hit/search", "hit/retest", "retest-chain>=8",
             "catchup/0", "catchup/1-3", "catchup/4", "catchup/5-64", "catchup/>64", "catchup/to-anchor",
             "catchup/to-start", "count/0", "count/1-19", "count/20", "count/21-275", "count/>275", "count/>262164",
             "count/to-matchlimit", "lit/0", "lit/1-14", "lit/15", "lit/16-255", "lit/256+", "lit/270", "ml/15",
             "ml/15+255", "off/1", "off/2-3", "off/65535", "far/rejected", "far/65536", "step>1", "step>acc",
             "end/search-ran-out", "end/match-at-mflimit", "last-literals/5", "sequences")
SNAPPY_NAMES = ("table/256", "table/512", "table/1024", "table/2048", "table/4096", "table/8192", "table/16384",
                "frag<15", "frags/1", "frags/2", "frags/>=4", "hit/search", "hit/retest", "probe>16", "probe/off>63",
                "search-ran-out", "end/copy", "copy1", "copy2/len>=12", "copy2/off>=2048", "copy/64", "copy/65-67",
                "copy/68", "copy/>=132", "lit/1-60", "lit/61-256", "lit/257-65536", "lit>256-before-copy",
                "lit/remainder")
LZ4_CLASSES = ["lz4/" + n for n in LZ4_NAMES]
SNAPPY_CLASSES = ["snappy/" + n for n in SNAPPY_NAMES]
ALL_CLASSES = LZ4_CLASSES + SNAPPY_CLASSES


def _counter(names, c):
    assert not c[len(names):].any(), "the restatement counts an event this file does not name"
    return Counter({n: int(v) for n, v in zip(names, c) if v})


def lz4(data, acc=1):
    """(compressed chunk, Counter) of one LZ4 chunk at that acceleration"""
    out, c = O.lz4_compress_census(data, acc)
    return out, _counter(LZ4_CLASSES, c)


def snappy(data):
    out, c = O.snappy_compress_census(data)
    return out, _counter(SNAPPY_CLASSES, c)


def snappy_tags(stream: bytes):
    """the tags of a snappy stream the restatement wrote: [("lit", length) | ("copy", length, offset)]"""
    ip = 0
    while stream[ip] & 128:
        ip += 1
    ip += 1
    tags = []
    while ip < len(stream):
        t = stream[ip]
        ip += 1
        if t & 3 == 0:
            ln = (t >> 2) + 1
            if ln > 60:
                nb = ln - 60
                ln = int.from_bytes(stream[ip:ip + nb], "little") + 1
                ip += nb
            tags.append(("lit", ln))
            ip += ln
        elif t & 3 == 1:
            tags.append(("copy", ((t >> 2) & 7) + 4, (t >> 5) << 8 | stream[ip]))
            ip += 1
        else:
            nb = 2 if t & 3 == 2 else 4
            tags.append(("copy", (t >> 2) + 1, int.from_bytes(stream[ip:ip + nb], "little")))
            ip += nb
    assert ip == len(stream)
    return tags


def census(codec, data, level=1):
    """(compressed chunk, Counter); codec lz4 / lz4fast (level = acceleration) / snappy"""
    return snappy(data) if codec == "snappy" else lz4(data, level if codec == "lz4fast" else 1)
