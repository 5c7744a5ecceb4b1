"""The constructed (dictionary, chunk) pairs of the zstd level-3 dictionary tests (include/lzbench_hip.h 3h): one pair
per branch of ZSTD_compressBlock_doubleFast_extDict_generic that lzh_debug_zstd_dfast_dict_parse counts, each with the
index of its event counter and, where the parse is predictable, one expected sequence.  The matrix of dictionaries and
chunks is tests/zstd_dict_inputs.py's.  Reads lzh_datagen and numpy alone."""
import numpy as np

import zstd_dict_inputs as I

LEVEL = 3
# the counters of lzh_debug_zstd_dfast_dict_parse (zfd::Event)
(REP_DICT, REP_CHUNK, LONG_DICT, LONG_CHUNK, SHORT_DICT, SHORT_CHUNK, LONG1_DICT, LONG1_CHUNK, REP2_DICT, REP2_CHUNK,
 CROSSED, BACK_DICT_START, BACK_CHUNK_START, REP_OVERLAP) = range(14)
NEVENTS = 14
EVENT_NAMES = ("rep-dict", "rep-chunk", "long-dict", "long-chunk", "short-dict", "short-chunk", "long1-dict",
               "long1-chunk", "rep2-dict", "rep2-chunk", "crossed", "back-dict-start", "back-chunk-start", "rep-overlap")
M64 = (1 << 64) - 1
rand = I.rand


def hash8(b8, hlog):
    return ((int.from_bytes(bytes(b8[:8]), "little") * 0xCF1BBCDCB7A56463) & M64) >> (64 - hlog)


def hash4(b4, hlog):
    return ((int.from_bytes(bytes(b4[:4]), "little") * 2654435761) & 0xFFFFFFFF) >> (32 - hlog)


def small_logs(total):
    """(hashLog, chainLog) of level 3 for n + dict_bytes = total <= 16384 (table 3, minMatch 4: srcLog + 1, srcLog)"""
    assert 64 <= total <= 16384
    s = int(np.ceil(np.log2(total)))
    return s + 1, s


def collide(target, hashf, hlog, width, seed):
    """`width` bytes whose hash under hashf at hlog equals target's and whose first byte differs"""
    rng = np.random.RandomState(seed)
    want = hashf(target, hlog)
    while True:
        t = rng.randint(0, 256, width).astype(np.uint8)
        if t[0] != target[0] and hashf(t, hlog) == want:
            return t


_cache = {}


def constructed():
    """{name: (dictionary, chunk, event, (sequence index, (ll, ml, offBase)) or None)}"""
    if _cache:
        return _cache
    c = _cache
    cat = np.concatenate
    dr = rand(4095, 5)                                   # 4095 = 3 x 1365: position D - 30 is indexed
    D = len(dr)
    a, b = 300, 900                                      # (multiples of 3: indexed)
    # the match starts 40 bytes before the dictionary's end and runs on into the chunk's start (two-segment count)
    d96 = rand(4096, 6)                                  # (4096 - 40 = 3 x 1352)
    c["cross"] = (d96, cat([d96[-40:], d96[-40:], rand(200, 7)]), CROSSED, (0, (0, 80, 40 + 3)))
    # catch-up that stops at the dictionary's first byte: index 2 (position 0) is never a match here
    # (matchIndex > dictStartIndex), so the chunk's copy of dict[0:] is found at position 3 and grows back to position 0
    d = rand(400, 8)
    c["catchup-dict-start"] = (d, cat([rand(6, 10), d[0:60], rand(100, 11)]), BACK_DICT_START,
                               (0, (6, 60, 6 + len(d) + 3)))
    # catch-up that stops at the chunk's first byte: position 0's bucket of the long table is taken by 8 colliding
    # bytes, its bucket of the short table by 4, so the repeat of r is found at position 1 and grows back to position 0
    r = rand(60, 12)
    d2 = rand(200, 13)
    hl, cl = small_logs(200 + 60 + 16 + 60 + 100)
    tl = collide(r[0:8], hash8, hl, 8, 14)
    ts = cat([collide(r[0:4], hash4, cl, 4, 15), rand(4, 16)])
    c["catchup-chunk-start"] = (d2, cat([r, tl, ts, r, rand(100, 17)]), BACK_CHUNK_START, (0, (76, 60, 76 + 3)))
    # a repcode at ip + 1 whose source lies in the dictionary / in the chunk: a match, one other byte, the source again
    mid = np.array([dr[a + 20] ^ 0x55], np.uint8)
    c["rep-in-dict"] = (dr, cat([dr[a: a + 20], mid, dr[a + 21: a + 60], rand(100, 18)]), REP_DICT, (1, (1, 39, 1)))
    q = rand(60, 19)
    midq = np.array([q[20] ^ 0x55], np.uint8)
    c["rep-in-chunk"] = (d2, cat([q, q[0:20], midq, q[21:60], rand(100, 20)]), REP_CHUNK, (1, (1, 39, 1)))
    # a repcode candidate whose source is the dictionary's last three bytes and the chunk's first: refused
    head = cat([dr[-30:-10], rand(7, 21)])
    c["rep-excluded"] = (dr, cat([head, dr[-3:], head[0:1], rand(60, 22)]), REP_OVERLAP, None)
    # the offset_2 loop with a source in the dictionary / in the chunk
    c["offset2-in-dict"] = (dr, cat([dr[a: a + 20], dr[b: b + 20], dr[a + 40: a + 60], rand(100, 23)]), REP2_DICT,
                            (2, (0, 20, 1)))
    q = rand(100, 24)
    c["offset2-in-chunk"] = (d2, cat([q, q[0:20], q[50:70], q[40:60], rand(100, 25)]), REP2_CHUNK, (2, (0, 20, 1)))
    # a long match with its source in the dictionary / in the chunk
    c["long-in-dict"] = (dr, cat([rand(10, 26), dr[b: b + 30], rand(100, 27)]), LONG_DICT,
                         (0, (10, 30, 10 + D - b + 3)))
    q = rand(50, 28)
    c["long-in-chunk"] = (d2, cat([q, rand(10, 29), q[10:40], rand(100, 30)]), LONG_CHUNK, (0, (60, 30, 50 + 3)))
    # a short match kept: six equal bytes, no eight anywhere
    c["short-in-dict"] = (dr, cat([rand(10, 31), dr[600:606], rand(100, 32)]), SHORT_DICT,
                          (0, (10, 6, 10 + D - 600 + 3)))
    q = rand(50, 33)
    c["short-in-chunk"] = (d2, cat([q, rand(10, 34), q[20:26], rand(100, 35)]), SHORT_CHUNK, (0, (60, 6, 40 + 3)))
    # a short match at ip and a long one at ip + 1, which is taken: the four bytes at 600 are one byte and the three
    # bytes that 1200 starts with
    dl = dr.copy()
    dl[1200:1203] = dl[601:604]
    c["long-at-ip1-in-dict"] = (dl, cat([rand(10, 36), dl[600:601], dl[1200:1230], rand(100, 37)]), LONG1_DICT,
                                (0, (11, 30, 11 + D - 1200 + 3)))
    q = rand(80, 38)
    q[40:43] = q[11:14]
    c["long-at-ip1-in-chunk"] = (d2, cat([q, rand(10, 39), q[10:11], q[40:70], rand(100, 40)]), LONG1_CHUNK,
                                 (0, (91, 30, 51 + 3)))
    # the largest offset: the chunk's last match reaches the dictionary's first byte (found at position 3, grown back)
    big = cat([rand(40, 41), np.zeros(131072 - 40, np.uint8)])
    c["largest-offset"] = (big, cat([I.chunk("text", 131072 - 20), big[0:20]]), BACK_DICT_START, None)
    # a chunk identical to the dictionary
    dj = I.dictionary("json", 4096)
    c["equal-4096"] = (dj, dj.copy(), LONG_DICT, None)
    # the 8-byte dictionary: referenced, not indexed
    d8 = I.dictionary("text", 8)
    c["dict-8"] = (d8, cat([d8, d8, I.chunk("text", 300)]), LONG_CHUNK, None)
    return c


def pairs():
    """{name: (dictionary, chunk)}"""
    return {k: v[:2] for k, v in constructed().items()}
