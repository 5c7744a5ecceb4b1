"""tests/zstd_dfast_cases.py -- the inputs of the zstd level-3 (double-fast) fixture, shared by its generator
(tests/golden/make_zstd_dfast_golden.py) and the tests that replay it.  A case is (name, corpus, n, chunk): the
corpus regenerates from (corpus, n, SEED); the constructed corpora are named for what they were built to contain,
which is a statement about the input, not about the branches a compressor takes on it."""
import numpy as np

import lzbench_amd as L

SEED = 5
LEVEL = 3


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def corpus(kind, n, seed=SEED):
    if kind == "zeros":                     # zero runs with a 7 every 4099 bytes: no block is one repeated byte
        d = np.zeros(n, np.uint8)
        d[::4099] = 7
        return d
    if kind == "zero":
        return np.zeros(n, np.uint8)
    if kind == "runs":
        rng = np.random.default_rng(seed)
        return np.repeat(rng.integers(0, 4, n // 8 + 16, dtype=np.uint8), rng.integers(1, 300, n // 8 + 16))[:n].copy()
    if kind == "random_block_then_text":    # a 128 KiB block that is stored raw, then text: repcodes left unconfirmed
        return np.concatenate([_rand(131072, seed), L.datagen("text", n - 131072, seed)])
    if kind == "far_copy_then_near_copy":   # random bytes, a copy of the first 64 KiB (beyond the 2 MiB window at
        a = n - 2 * 65536                   # chunk sizes over 2 MiB), then a copy of the 64 KiB before that copy
        r = _rand(a, seed)
        return np.concatenate([r, r[:65536], r[a - 65536:a]])
    if kind == "repeat_after_incompressible":   # 1500 random bytes directly before a repeat of earlier text
        t = L.datagen("text", 8192, seed)
        return np.concatenate([t, _rand(1500, seed), t[1000:3000], _rand(700, seed + 1), t[4000:4100]])[:n]
    if kind == "runs_68_sequences":          # 16 KiB of byte runs that parse into 68 sequences: between 64 and 72, where
        return corpus("runs", 1 << 19, 4)[325127:325127 + n].copy()   # fast and double-fast pick other table types
    if kind == "period3":
        return np.tile(np.frombuffer(b"abc", np.uint8), n // 3 + 1)[:n].copy()
    if kind == "period5":                   # period 5 with one foreign byte in the middle
        d = np.tile(np.frombuffer(b"abcde", np.uint8), n // 5 + 1)[:n].copy()
        d[n // 2] = ord("x")
        return d
    return L.datagen(kind, n, seed)


def cases():
    c = []
    for n in (0, 1, 7, 8, 9, 12, 63, 64, 65, 1023):              # ilimit, the source-log clamp, the window minimum
        c.append((f"text-{n}", "text", n, 131072))
    for n in (16384, 16385, 131072, 131073, 262144, 262145):     # the table boundaries, one block / two blocks
        for kind in ("text", "mixed"):
            c.append((f"{kind}-{n}", kind, n, n))
    for kind in ("text", "json", "binary", "mixed", "runs", "zeros", "zero", "random"):
        c.append((f"{kind}-300000-one-chunk", kind, 300_000, 524288))    # three blocks, tables and repcodes carried
        c.append((f"{kind}-b64-ragged-tail", kind, 3 * 65536 + 12345, 65536))
    c.append(("random-block-then-text", "random_block_then_text", 131072 + 70_000, 262144))
    c.append(("zero-262145", "zero", 262_145, 262_145))          # RLE blocks
    c.append(("far-copy-then-near-copy-b4096", "far_copy_then_near_copy", 2400 * 1024 + 517 + 2 * 65536, 4 << 20))
    c.append(("repeat-after-incompressible", "repeat_after_incompressible", 8192 + 1500 + 2000 + 700 + 100, 131072))
    c.append(("runs-68-sequences", "runs_68_sequences", 16384, 16384))
    c.append(("period3-5000", "period3", 5000, 131072))
    c.append(("period5-5000", "period5", 5000, 131072))
    return c


def chunk_list(n, chunk):
    """the chunk sizes of a case: lzbench's list, and one empty chunk for the empty input"""
    return np.zeros(1, np.uint64) if n == 0 else L.chunk_sizes_for(n, chunk)
