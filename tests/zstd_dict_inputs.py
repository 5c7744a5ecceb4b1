"""Named, seeded, small inputs of the zstd dictionary tests (include/lzbench_hip.h 3f): dictionaries and chunks cut
from lzh_datagen's corpora, and the constructed (dictionary, chunk) pairs that reach the branches of the extDict parse.
Reads lzh_datagen and numpy alone."""
import numpy as np

import lzbench_amd as L

DICT_SIZES = (8, 9, 11, 4095, 4096, 65536, 112640, 131072)
CHUNK_SIZES = (0, 1, 6, 7, 8, 9, 64, 300, 1000, 4099, 16384, 70000, 131072)
BOUNDARIES = (16384, 16385, 131072, 131073, 262144)      # n + dict_bytes where ZSTD_getParams changes its row
KINDS = ("text", "json")
LEVELS = (1, -3)
MAXD = 131072
_SEED = {"json": 51, "text": 53}
_streams = {}


def _stream(kind):
    """128 KiB that the dictionaries are cut from (their last bytes), then the bytes the chunks are cut from."""
    if kind not in _streams:
        _streams[kind] = L.datagen(kind, MAXD + 900000, seed=_SEED[kind])
    return _streams[kind]


def dictionary(kind: str, size: int) -> np.ndarray:
    return _stream(kind)[MAXD - size: MAXD].copy()


def boundary_sizes(dict_bytes: int):
    """the chunk sizes that put n + dict_bytes on a table boundary, within the limits"""
    return [t - dict_bytes for t in BOUNDARIES if 1 <= t - dict_bytes <= 131072]


def chunk_sizes(dict_bytes: int):
    return sorted(set(CHUNK_SIZES) | set(boundary_sizes(dict_bytes)))


def chunk(kind: str, size: int, slot: int = 0) -> np.ndarray:
    """`size` bytes of the corpus after the dictionary's, from a place that depends on the size"""
    at = MAXD + 11 + (size * 7 + slot * 3001) % 600000
    return _stream(kind)[at: at + size].copy()


def rand(n, seed):
    return L.datagen("random", n, seed=seed).copy()


def chunks(kind: str, dict_bytes: int):
    """[(name, bytes)]: every size as the dictionary's vocabulary, as random bytes (stored raw) and as zeros"""
    out = []
    for s in chunk_sizes(dict_bytes):
        out.append((f"{kind}-{s}", chunk(kind, s)))
        out.append((f"random-{s}", rand(s, 100 + s % 89)))
        out.append((f"zeros-{s}", np.zeros(s, np.uint8)))
    return out


def dictionaries():
    """[(name, kind, bytes)]: every size from both corpora"""
    return [(f"{k}-{s}", k, dictionary(k, s)) for s in DICT_SIZES for k in KINDS]


def records(kind: str, count: int, size: int):
    """`count` records of about `size` bytes (size - 8 .. size + 7) of one corpus"""
    return [chunk(kind, size - 8 + i % 16, slot=i + 1) for i in range(count)]


# ---- the constructed pairs -------------------------------------------------------------------------------------
def _hash5(b8, hlog):
    v = int.from_bytes(bytes(b8[:8]), "little")
    return (((v << 24) & (2 ** 64 - 1)) * 889523592379 & (2 ** 64 - 1)) >> (64 - hlog)


def collide(target8, hlog, seed):
    """8 bytes whose 5-byte hash at hashLog `hlog` equals target8's and whose first byte differs"""
    rng = np.random.RandomState(seed)
    want = _hash5(target8, hlog)
    while True:
        t = rng.randint(0, 256, 8).astype(np.uint8)
        if t[0] != target8[0] and _hash5(t, hlog) == want:
            return t


def _hlog_small(total):
    """hashLog of levels 1 and -3 alike for n + dict_bytes = total <= 4096 (table 3: srcLog + 1 below both rows)"""
    assert 64 <= total <= 4096
    return int(np.ceil(np.log2(total))) + 1


def constructed():
    """{name: (dictionary, chunk)}, each built for one branch of ZSTD_compressBlock_fast_extDict_generic at level 1
    (tests/test_zstd_dict_ref.py reads the branch off the host walk's sequences)."""
    c = {}
    dr = rand(4095, 5)                                   # 4095 = 3 x 1365: position D - 30 is indexed
    # the match starts 40 bytes before the dictionary's end and runs on into the chunk's start (two-segment count)
    d96 = rand(4096, 6)                                  # (4096 - 40 = 3 x 1352)
    c["cross"] = (d96, np.concatenate([d96[-40:], d96[-40:], rand(200, 7)]))
    # catch-up that stops at the dictionary's first byte: position 0's bucket is taken by a later position with the
    # same hash (T at 300), so the chunk's copy of dict[0:] is found at position 3 and grows back to position 0
    n1 = 6 + 60 + 100
    d = rand(400, 8)
    d[300:308] = collide(d[0:8], _hlog_small(400 + n1), 9)
    c["catchup-dict-start"] = (d, np.concatenate([rand(6, 10), d[0:60], rand(100, 11)]))
    # catch-up that stops at the chunk's first byte: the same with a colliding 8 bytes inside the chunk
    r = rand(60, 12)
    n2 = 60 + 8 + 60 + 100
    d2 = rand(200, 13)
    t = collide(r[0:8], _hlog_small(200 + n2), 14)
    c["catchup-chunk-start"] = (d2, np.concatenate([r, t, r, rand(100, 15)]))
    # a repcode at ip + 1 whose source lies in the dictionary: a match to the dictionary, one other byte, the
    # dictionary again at the same offset
    a = 300
    mid = np.array([dr[a + 20] ^ 0x55], np.uint8)
    c["rep-in-dict"] = (dr, np.concatenate([dr[a: a + 20], mid, dr[a + 21: a + 60], rand(100, 16)]))
    # a repcode candidate whose source is the dictionary's last three bytes and the chunk's first: excluded
    head = np.concatenate([dr[-30:-10], rand(7, 17)])
    c["rep-excluded"] = (dr, np.concatenate([head, dr[-3:], head[0:1], rand(60, 18)]))
    # the offset_2 loop with a source in the dictionary
    b = 900
    c["offset2-in-dict"] = (dr, np.concatenate([dr[a: a + 20], dr[b: b + 20], dr[a + 40: a + 60], rand(100, 19)]))
    # the largest offset: the chunk's last match reaches the dictionary's first byte
    # (the dictionary is 40 random bytes and then zeros: a full random one overwrites position 0's bucket, the largest
    # index of a bucket wins)
    big = np.concatenate([rand(40, 20), np.zeros(131072 - 40, np.uint8)])
    c["largest-offset"] = (big, np.concatenate([chunk("text", 131072 - 20), big[0:20]]))
    # a chunk identical to the dictionary
    dj = dictionary("json", 4096)
    c["equal-4096"] = (dj, dj.copy())
    # the 8-byte dictionary: referenced, not indexed
    d8 = dictionary("text", 8)
    c["dict-8"] = (d8, np.concatenate([d8, d8, chunk("text", 300)]))
    return c
