"""LZ4 parse, the end of a chunk and the collision-free resolve: the run batch's resolve is compiled three times
(lz4c.h: far from the chunk's end with and without in-batch slot collisions, and the tail with every end-of-chunk
term), selected per batch by uniform tests.  Chunk sizes either side of every limit those tests and the tail use
(MINLENGTH 13, one batch, mflimit 12 / matchlimit 5 before the end, the 24-byte candidate window plus the 64 lanes
= 88, the byU16 / byU32 switch at 65 547), on inputs whose matches run into the limits, as one chunk and as the short
last chunk after two full ones: packed bytes and compr_sizes against the CPU checker (the reference build where
it is present, else the restatement), and a round trip through the decoder.  Run with -m gpu."""
import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
from gpu_batches import torch_cuda

pytestmark = pytest.mark.gpu

SIZES = ([13, 64, 65, 76, 77] + list(range(83, 97)) + [128 + d for d in (-13, -12, -1, 0, 1, 12, 13)]
         + [4096 - 13, 4096 + 13] + [65536 - d for d in (0, 1, 5, 12, 13, 24, 25, 88, 89)] + [65546, 65547])


def _run_to(n, k):
    """text, then one byte repeated up to k bytes before the end, then k distinct bytes"""
    d = L.datagen("text", n, seed=5).copy()
    a = n // 4
    if n - k > a:
        d[a:n - k] = 0x61
        d[n - k:] = np.arange(1, k + 1, dtype=np.uint8)
    return d


INPUTS = {
    "text": lambda n: L.datagen("text", n, seed=3),
    "period3": lambda n: np.resize(np.frombuffer(b"abc", np.uint8), n).copy(),
    "period64": lambda n: np.resize(L.datagen("random", 64, seed=9), n).copy(),
    "run_to_12": lambda n: _run_to(n, 12),
    "run_to_5": lambda n: _run_to(n, 5),
    "run_to_4": lambda n: _run_to(n, 4),
    "random": lambda n: L.datagen("random", n, seed=7),
}


def _hash13(w):   # LZ4_hash4 with the byU16 table's 13 bits (lz4.c:751-757)
    return ((w * 2654435761) & 0xFFFFFFFF) >> 19


def no_collision_chunk(n, seed):
    """bytes with matches (copies of earlier pieces) in which no two of any 64 consecutive positions share a table
    slot: each new byte is taken only if its 4-gram's slot differs from the 63 slots before it"""
    rng = np.random.default_rng(seed)
    out = bytearray(n)
    slots = []                  # slot of the 4-gram starting at each position
    recent = {}
    src, left = 0, 0
    fresh = rng.integers(0, 256, size=(n, 6))
    plan = rng.integers(0, 1 << 30, size=(n, 2))
    for i in range(n):
        if left == 0 and i > 200 and plan[i, 0] % 12 == 0:
            src, left = int(plan[i, 1] % (i - 100)), 6 + int(plan[i, 0] >> 8) % 24
        cands = ([out[src]] if left else []) + [int(b) for b in fresh[i]]
        took = None
        for j, b in enumerate(cands):
            if i < 3:
                took = b
                break
            h = _hash13(out[i - 3] | out[i - 2] << 8 | out[i - 1] << 16 | b << 24)
            if h not in recent:
                took, hh = b, h
                if not (left and j == 0):
                    left = 0
                break
        assert took is not None
        out[i] = took
        if left:
            src, left = src + 1, left - 1
        if i >= 3:
            slots.append(hh)
            recent[hh] = 1
            if len(slots) > 63:
                del recent[slots[-64]]
    return np.frombuffer(bytes(out), np.uint8).copy()


def colliding_chunk(n, seed):
    """the same 4-gram at distance 8 throughout: every batch has lanes that share its slot"""
    d = L.datagen("random", n, seed=seed).copy()
    for k in range(4):
        d[k::8] = b"LZ4!"[k]
    return d


def _check(torch, data, chunk):
    n = len(data)
    d_in = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(torch.from_numpy(data))
    dc = L.DeviceCodec("lz4", n, chunk)
    dc.compress(d_in)
    dc.decompress()
    torch.cuda.synchronize()
    exp_packed, exp_cs = O.compress_chunks(data, "lz4", chunk, use_ref=O.have_ref())
    cs = dc.csizes.cpu().numpy().astype(np.uint64)
    if not (len(cs) == len(exp_cs) and (cs == exp_cs).all()):
        return f"compr_sizes {cs.tolist()} != {exp_cs.tolist()}"
    total = dc.packed_total()
    if total != len(exp_packed) or not (dc.packed[:total].cpu().numpy() == exp_packed).all():
        return "packed bytes differ"
    if not (dc.status.cpu().numpy() >= 0).all() or not (dc.out[:n].cpu().numpy() == data).all():
        return "round trip failed"
    return None


@pytest.mark.parametrize("layout", ["single", "last_of_three"])
@pytest.mark.parametrize("kind", list(INPUTS))
def test_chunk_end_sizes(torch_cuda, kind, layout):
    bad = []
    for s in SIZES:
        if layout == "single":
            n, chunk = s, s
        elif s <= 65536:
            n, chunk = 2 * 65536 + s, 65536     # two full 64 KiB chunks, then s bytes
        else:
            n, chunk = 3 * s, s                 # (past 64 KiB: three chunks of s bytes)
        why = _check(torch_cuda, INPUTS[kind](n), chunk)
        if why:
            bad.append((s, why))
    assert not bad, bad


@pytest.mark.parametrize("make", [no_collision_chunk, colliding_chunk], ids=["no_collision", "all_collide"])
def test_collision_free_and_colliding_batches(torch_cuda, make):
    data = make(65536, 21)
    if make is no_collision_chunk:   # the construction holds: 64 consecutive positions, 64 slots
        w = data[:-3].astype(np.uint64) | data[1:-2].astype(np.uint64) << 8 | data[2:-1].astype(np.uint64) << 16 \
            | data[3:].astype(np.uint64) << 24
        h = _hash13(w)
        for d in range(1, 64):
            assert not (h[d:] == h[:-d]).any()
    assert _check(torch_cuda, data, 65536) is None
    two = np.concatenate([data, make(65536 - 25, 22)])
    assert _check(torch_cuda, two, 65536) is None
