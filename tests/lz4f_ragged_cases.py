"""What the ragged LZ4 frame tests share (include/lzbench_hip.h 3i): the per-frame oracle with the raw-store rule, the
bit-exactness batch, and the corrupted frames of the verdict test.  A plain module: no tests.  The references are the
restatement's LZ4F_compressFrame / LZ4F_decompress (oracle/frame_oracle.c, pinned to the reference build by
tests/test_frames.py), never the code under test."""
import numpy as np

import frame_cases as F
import lzbench_amd as L
import oracle_lib as O

LINKED = L.LZ4F_LINKED
# the sizes of the bit-exactness batch: empty, below and at LZ4's 13-byte limit, around one and two 64 KiB blocks,
# the largest chunk; the two random chunks sit at one block and one block plus a byte
SIZES = (0, 1, 12, 13, 4096, 65535, 65536, 65537, 131072, 131073, 200000, 262144)
KINDS = ("text", "json", "mixed", "binary")
VERDICT_LEVELS = (0, 0x10, 0x20, 0x40, 0x70, 5, 0x80, 0xB0)
VERDICT_SEED, VERDICT_FRAMES, VERDICT_SIZE = 20, 200, 70000


def frame(data: np.ndarray, params: int) -> bytes:
    """the frame oracle_lz4f_compress writes for data alone (params & LINKED: linked blocks)"""
    orc = O.oracle()
    data = np.ascontiguousarray(data, dtype=np.uint8)
    src = data if len(data) else np.zeros(1, np.uint8)
    out = np.zeros(int(orc.oracle_lz4f_bound(len(data), params)) + 64, np.uint8)
    r = orc.oracle_lz4f_compress(src.ctypes.data, len(data), out.ctypes.data, params)
    assert r > 0, (r, params)
    return out[:r].tobytes()


def stored(data: np.ndarray, params: int) -> bytes:
    """the bytes a compress call packs for the chunk: its frame, or the chunk itself where the two have one size"""
    f = frame(data, params)
    return data.tobytes() if len(f) == len(data) else f


def decode(s: bytes, n: int):
    """(oracle_lz4f_decompress's answer for a frame that must decode to n bytes, its output)"""
    src = np.frombuffer(s, np.uint8).copy() if len(s) else np.zeros(1, np.uint8)
    dst = np.zeros(n + 64, np.uint8)
    r = int(O.oracle().oracle_lz4f_decompress(src.ctypes.data, len(s), dst.ctypes.data, n))
    return r, dst[:max(r, 0)]


def batch_parts(sizes=SIZES, seed=3):
    """chunks of `sizes`, the corpus kinds in turn; the chunks of 65536 and 65537 bytes are random (blocks stored raw)"""
    parts = []
    for i, n in enumerate(sizes):
        kind = "random" if n in (65536, 65537) else KINDS[i % len(KINDS)]
        parts.append(L.datagen(kind, n, seed=seed + i))
    return parts


def corrupted_frames():
    """[(frame bytes, level)]: VERDICT_FRAMES corruptions of the frames of one 70000-byte text chunk, a fixed seed"""
    rng = np.random.default_rng(VERDICT_SEED)
    data = L.datagen("text", VERDICT_SIZE, seed=9)
    good = {p: frame(data, p) for p in VERDICT_LEVELS}
    out = []
    for _ in range(VERDICT_FRAMES):
        p = int(rng.choice(VERDICT_LEVELS))
        out.append((F.corrupt(rng, good[p]), p))
    return data, out
