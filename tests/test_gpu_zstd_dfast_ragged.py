"""GPU: ragged zstd level-3 batches (include/lzbench_hip.h 3e, lzbench_amd.RaggedCodec("zstd_dfast")) -- per-chunk
pointers and sizes through the uniform-slot and the compact layout against the committed reference digests
(tests/golden/zstd_dfast_golden.json), the uniform call, the reference build frame by frame, the ragged decoders, and
the guards of the two calls.  Run with -m gpu."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
import zstd_dfast_cases as Z
from gpu_batches import SLACK, layout, roundtrip, sha, to_dev, torch_cuda
from zstd_ragged_inputs import corpus_mix

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ["uniform", "compact"]
FAR = "far-copy-then-near-copy-b4096"
# the ZSTD_getParams size classes and the block boundaries, each with its neighbours
BOUNDARY = [s + d for s in (64, 16384, 131072, 262144) for d in (-1, 0, 1)]


def codec(mode, maxb, k, total=None, **kw):
    return L.RaggedCodec("zstd_dfast", maxb, k, level=3, max_total_bytes=total, compact_scratch=mode == "compact", **kw)


def result(torch, rc, k):
    """(csizes, offsets, packed bytes) of rc's last compress call, the offsets checked against the sizes"""
    torch.cuda.synchronize()
    cs = rc.csizes[:k].cpu().numpy().astype(np.int64)
    of = rc.offsets[: k + 1].cpu().numpy()
    assert (of == np.concatenate([[0], np.cumsum(cs)])).all(), "offsets are not the exclusive scan of csizes"
    return cs, of, rc.packed[: int(of[k])].cpu().numpy()


def frames(cs, of, packed):
    return [packed[of[i]: of[i + 1]].tobytes() for i in range(len(cs))]


def decode_both(torch, rc, host, offs, sizes, skip=()):
    """the round trip through lzh_zstd_decompress_ragged_async: one-wave, and with the split decoder's temp where the
    chunk size has one"""
    roundtrip(torch, rc, host, offs, sizes, skip=skip)
    dt = L.lib().lzh_zstd_ragged_decompress_split_temp_bytes(rc.max_chunk_bytes, rc.max_chunks)
    assert (dt > 0) == (rc.max_chunk_bytes >= 16384)
    if dt:
        small, rc.dtemp = rc.dtemp, torch.empty(dt, dtype=torch.uint8, device="cuda")
        assert dt > small.numel()
        roundtrip(torch, rc, host, offs, sizes, skip=skip)
        rc.dtemp = small


# ---- 1. the committed digests: every one-chunk case of the level-3 fixture as the chunks of one batch -------------
@pytest.fixture(scope="module")
def golden_batch():
    with open(os.path.join(GOLD, "zstd_dfast_golden.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["chunk"] >= c["n"]]
    names = [c["name"] for c in cases]
    for n in (0, 1, 7, 8, 9, 12, 63, 64, 65, 1023):
        assert f"text-{n}" in names
    for n in (16384, 16385, 131072, 131073, 262144, 262145):
        assert f"text-{n}" in names and f"mixed-{n}" in names
    assert "runs-68-sequences" in names and "period3-5000" in names and "period5-5000" in names
    assert sum(c["n"] == 300_000 for c in cases) == 8 and FAR in names
    far = cases[names.index(FAR)]
    cases = [c for c in cases if c["name"] != FAR]
    sizes = [c["n"] for c in cases]
    offs, total = layout(sizes, residues=(0, 1, 2, 3))
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    host = np.full(total, 0x5A, np.uint8)
    for c, o in zip(cases, offs):
        data = Z.corpus(c["corpus"], c["n"], c["seed"])
        assert sha(data) == c["input_sha256"]
        host[o: o + c["n"]] = data
    return cases, far, host, offs, sizes


def check_golden(cases, cs, of, packed):
    for i, c in enumerate(cases):
        assert int(cs[i]) == c["packed_bytes"], (c["name"], int(cs[i]))
        assert sha(packed[of[i]: of[i + 1]]) == c["packed_sha256"], c["name"]


@pytest.mark.parametrize("mode", MODES)
def test_fixture_frames_in_one_batch(torch_cuda, golden_batch, mode):
    torch = torch_cuda
    cases, _, host, offs, sizes = golden_batch
    rc = codec(mode, max(sizes), len(sizes), sum(sizes))
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, packed = result(torch, rc, len(sizes))
    check_golden(cases, cs, of, packed)
    assert int(cs[sizes.index(0)]) == 9                 # the empty chunk's frame
    decode_both(torch, rc, host, offs, sizes)


def test_matches_beyond_the_window(torch_cuda, golden_batch):
    """the 2.5 MiB case, the one input whose matches pass the 2 MiB window: one chunk, uniform slots"""
    torch = torch_cuda
    far = golden_batch[1]
    host = np.concatenate([np.zeros(3, np.uint8), Z.corpus(far["corpus"], far["n"], far["seed"]), np.zeros(SLACK, np.uint8)])
    rc = codec("uniform", far["n"], 1)
    rc.compress(to_dev(torch, host), [3], [far["n"]])
    cs, of, packed = result(torch, rc, 1)
    check_golden([far], cs, of, packed)
    decode_both(torch, rc, host, [3], [far["n"]])


# ---- 2. equals the uniform call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", [16384, 131072])
def test_equals_the_uniform_call(torch_cuda, chunk, mode):
    torch = torch_cuda
    n = (2 << 20) + 333
    host = corpus_mix(n, 3)
    d_in = to_dev(torch, host, SLACK)
    dc = L.DeviceCodec("zstd_dfast", n, chunk, 3)
    dc.compress(d_in)
    sizes = L.chunk_sizes_for(n, chunk).astype(np.int64)
    offs = np.arange(len(sizes), dtype=np.int64) * chunk
    k = len(sizes)
    rc = codec(mode, chunk, k, n)
    rc.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    assert dc.k == k
    assert torch.equal(rc.csizes[:k], dc.csizes) and torch.equal(rc.offsets[: k + 1], dc.offsets)
    total = dc.packed_total()
    assert rc.packed_total() == total and torch.equal(rc.packed[:total], dc.packed[:total])
    decode_both(torch, rc, host, offs, [int(s) for s in sizes])


# ---- 3. the reference build, frame by frame ------------------------------------------------------------------------
_ref_batches = None


def ref_batches():
    """twelve seeded batches of 16 slices (sizes 1 .. 300,000 and the boundary sizes) with the reference build's frames"""
    global _ref_batches
    if _ref_batches is None:
        rng = np.random.default_rng(44)
        src = np.concatenate([L.datagen("mixed", 1 << 21, seed=3), Z.corpus("runs", 1 << 19, 4),
                              rng.integers(0, 3, 1 << 18, dtype=np.uint8), L.datagen("json", 1 << 20, seed=1)])
        out = []
        for b in range(12):
            sizes = [int(rng.choice(BOUNDARY)) if rng.random() < 0.4 else int(rng.integers(1, 300_001)) for _ in range(16)]
            starts = [int(rng.integers(0, len(src) - s)) for s in sizes]
            offs, total = layout(sizes, residues=(b % 4, 3, 2, 1, 0))
            host = np.zeros(total, np.uint8)
            expect = []
            for s, a, o in zip(sizes, starts, offs):
                part = src[a: a + s].copy()
                host[o: o + s] = part
                p, cs = O.compress_chunks(part, "zstd", s, 3, use_ref=True)
                assert len(cs) == 1 and int(cs[0]) == len(p)
                expect.append(p.tobytes())
            out.append((host, offs, sizes, expect))
        _ref_batches = out
    return _ref_batches


@pytest.mark.parametrize("mode", MODES)
def test_random_batches_equal_reference_build(torch_cuda, mode):
    torch = torch_cuda
    if not O.have_ref():
        pytest.skip("reference build (oracle/_ref) not present")
    rc = codec(mode, 300_000, 16)
    for b, (host, offs, sizes, expect) in enumerate(ref_batches()):
        rc.compress(to_dev(torch, host), offs, sizes)
        got = frames(*result(torch, rc, 16))
        for i in range(16):
            assert got[i] == expect[i], f"batch {b} chunk {i} ({sizes[i]} bytes)"
        decode_both(torch, rc, host, offs, sizes)


# ---- 4. guards -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_oversize_chunk_is_not_processed(torch_cuda, mode):
    torch = torch_cuda
    maxb = 140000                               # (two blocks: the second launch must skip the chunk as well)
    sizes = [3000, maxb + 1, maxb, 17]          # entry 1 is one byte too large (and really that large)
    offs, total = layout(sizes)
    host = corpus_mix(total, 17)
    d_in = to_dev(torch, host)
    good = [0, 2, 3]
    clean = codec(mode, maxb, 3)
    clean.compress(d_in, offs[good], [sizes[i] for i in good])
    want = frames(*result(torch, clean, 3))
    rc = codec(mode, maxb, len(sizes), sum(sizes))
    # the temp buffer is exactly the sizing answer, the packed buffer exactly max_packed; guard bytes on both sides
    G = 4096
    lib = L.lib()
    ct = (lib.lzh_zstd_dfast_ragged_compact_compress_temp_bytes(3, sum(sizes), maxb, 4) if mode == "compact"
          else lib.lzh_zstd_dfast_ragged_compress_temp_bytes(3, maxb, 4))
    assert ct == rc.ctemp.numel()
    temp = torch.full((ct + 2 * G,), 0xEE, dtype=torch.uint8, device="cuda")
    packed = torch.full((rc.max_packed + 2 * G,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.ctemp, rc.packed = temp[G: G + ct], packed[G: G + rc.max_packed]
    rc.compress(d_in, offs, sizes)
    cs, of, pk = result(torch, rc, 4)
    got = frames(cs, of, pk)
    assert int(cs[1]) == 0 and of[1] == of[2] and [got[i] for i in good] == want
    assert bool((temp[:G] == 0xEE).all()) and bool((temp[G + ct:] == 0xEE).all()), "write outside the temp buffer"
    assert bool((packed[:G] == 0xEE).all()) and bool((packed[G + int(of[4]):] == 0xEE).all()), "write outside packed"
    if mode == "uniform":
        # the oversize chunk's staging slot (slot 1) and scratch area (area 1) were not touched; its neighbours' were
        stride = lib.lzh_stage_stride(L.LZH_CODEC_ZSTD, maxb)
        area = ct // 4 - stride                 # (temp_layout.h zstd_dfast_ragged_temp: the slots, then the areas)
        a0 = G + 4 * stride
        assert bool((temp[G + stride: G + 2 * stride] == 0xEE).all()), "the oversize chunk's staging slot was written"
        assert area > maxb and bool((temp[a0 + area: a0 + 2 * area] == 0xEE).all()), "the oversize chunk's scratch was written"
        assert not bool((temp[a0: a0 + area] == 0xEE).all()) and not bool((temp[a0 + 2 * area: a0 + 3 * area] == 0xEE).all())
    else:
        # the oversize chunk has slots of 0 bytes: its neighbours' slots are adjacent, as the mirror places them
        a = (C.c_uint64 * 4)(*sizes)
        so, ro, pr = (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint8 * 4)()
        assert lib.lzh_debug_zstd_dfast_ragged_compact_slots(3, a, 4, maxb, sum(sizes), so, ro, pr) == 0
        assert list(pr) == [1, 0, 1, 1] and so[1] == so[2] and ro[1] == ro[2]
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})
    assert int(st[1]) == -1


@pytest.mark.parametrize("mode", MODES)
def test_temp_and_packed_cap_guards(torch_cuda, mode):
    torch = torch_cuda
    sizes = [70000, 5, 16385, 0, 131073, 4099]
    offs, total = layout(sizes)
    host = corpus_mix(total, 31)
    k = len(sizes)
    rc = codec(mode, max(sizes), k, sum(sizes))
    d_in = to_dev(torch, host)
    rc.compress(d_in, offs, sizes)
    cs, of, full = result(torch, rc, k)
    # a temp_bytes one byte short: LZH_ESPACE before any launch (the outputs stay as they are)
    whole = rc.ctemp
    rc.ctemp = whole[: whole.numel() - 1]
    rc.csizes.fill_(-7)
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        rc.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    assert bool((rc.csizes == -7).all())
    # temp of exactly the sizing answer, followed by guard bytes that stay as they are
    G = 4096
    ct = whole.numel()
    ctemp = torch.full((ct + G,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.ctemp = ctemp[:ct]
    # a packed_cap below the total: chunks whose range would pass it are not written, the sizes are all reported
    cap = int(of[4]) + 100                       # inside chunk 4's frame
    big = torch.full((int(of[k]) + G,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.packed = big[:cap]
    rc.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    assert (rc.csizes[:k].cpu().numpy() == cs).all() and (rc.offsets[: k + 1].cpu().numpy() == of).all()
    assert rc.packed_total() > cap               # d_offsets[nchunks]: the caller learns that the output is incomplete
    got = big.cpu().numpy()
    assert (got[: of[4]] == full[: of[4]]).all(), "chunks below the cap"
    assert (got[cap:] == 0xEE).all(), "bytes past packed_cap were written"
    assert bool((ctemp[ct:] == 0xEE).all()), "write past the compress temp"


def test_compact_batch_that_breaks_its_promise(torch_cuda):
    torch = torch_cuda
    sizes = [20000, 4099, 131073, 0, 70000, 300, 16385, 9000, 64, 50000]
    offs, total = layout(sizes)
    host = corpus_mix(total, 37)
    d_in = to_dev(torch, host)
    k, maxb = len(sizes), max(sizes)
    honest = codec("compact", maxb, k, sum(sizes))
    honest.compress(d_in, offs, sizes)
    want = frames(*result(torch, honest, k))
    promise = 100_000                            # (the batch has three times as much)
    a = (C.c_uint64 * k)(*sizes)
    so, ro, pr = (C.c_uint64 * k)(), (C.c_uint64 * k)(), (C.c_uint8 * k)()
    assert L.lib().lzh_debug_zstd_dfast_ragged_compact_slots(3, a, k, maxb, promise, so, ro, pr) == 0
    named = [i for i in range(k) if not pr[i]]
    assert 0 < len(named) < k
    rc = codec("compact", maxb, k, promise)
    G = 4096
    ct = rc.ctemp.numel()
    temp = torch.full((ct + 2 * G,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.ctemp, rc.packed = temp[G: G + ct], honest.packed.clone()
    d, _ = honest._arrays(d_in, offs, sizes, 16)   # (device arrays made without the promise's host check)
    rc.compress_arrays(d, k)
    cs, of, pk = result(torch, rc, k)
    got = frames(cs, of, pk)
    for i in range(k):
        assert got[i] == (b"" if i in named else want[i]), f"chunk {i}"
    assert bool((temp[:G] == 0xEE).all()) and bool((temp[G + ct:] == 0xEE).all()), "write outside the temp buffer"


@pytest.mark.parametrize("mode", MODES)
def test_a_smaller_batch_after_a_larger_one(torch_cuda, golden_batch, mode):
    """one RaggedCodec, its temp reused: the tables are zeroed per frame, whatever the slot held before"""
    torch = torch_cuda
    cases, _, host, offs, sizes = golden_batch
    rc = codec(mode, max(sizes), len(sizes), sum(sizes))
    d_in = to_dev(torch, host)
    rc.compress(d_in, offs, sizes)
    check_golden(cases, *result(torch, rc, len(sizes)))
    pick = [i for i in np.random.default_rng(9).permutation(len(sizes)) if sizes[i] <= 131073][:11]
    rc.compress(d_in, offs[pick], [sizes[i] for i in pick])
    check_golden([cases[i] for i in pick], *result(torch, rc, len(pick)))


# ---- 5. a skewed batch ---------------------------------------------------------------------------------------------
def test_skewed_batch(torch_cuda):
    torch = torch_cuda
    lib = L.lib()
    sizes = [4096] * 255 + [1 << 20]
    k, maxb, total = 256, 1 << 20, sum(sizes)
    ct, ut = (lib.lzh_zstd_dfast_ragged_compact_compress_temp_bytes(3, total, maxb, k),
              lib.lzh_zstd_dfast_ragged_compress_temp_bytes(3, maxb, k))
    assert 10 * ct < ut                          # (host arithmetic: before anything is allocated)
    offs, n = layout(sizes)
    host = corpus_mix(n, 51)
    d_in = to_dev(torch, host)
    a, b = codec("compact", maxb, k, total), codec("uniform", maxb, k, total)
    assert a.ctemp.numel() == ct and b.ctemp.numel() == ut
    a.compress(d_in, offs, sizes)
    b.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    assert torch.equal(a.csizes, b.csizes) and torch.equal(a.offsets, b.offsets)
    t = a.packed_total()
    assert 0 < t == b.packed_total() and torch.equal(a.packed[:t], b.packed[:t])
    assert int(a.csizes.min()) > 0
    decode_both(torch, a, host, offs, sizes)


# ---- 6. graph capture ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_graph_replay(torch_cuda, mode):
    torch = torch_cuda
    sizes = [70000, 0, 13, 4099, 131073, 9]
    offs, total = layout(sizes)
    d_in = to_dev(torch, corpus_mix(total, 29))
    rc, eager = codec(mode, max(sizes), len(sizes)), codec(mode, max(sizes), len(sizes))
    d_src, k = rc._arrays(d_in, offs, sizes, 16)
    eager.compress_arrays(d_src, k)              # (the kernels' code is loaded before the capture begins)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):       # captured on a non-default stream
        rc.compress_arrays(d_src, k)
    seen = []
    for seed in (61, 62):                        # each replay over other input bytes at the same addresses
        d_in.copy_(to_dev(torch, corpus_mix(total, seed)))
        for t in (rc.packed, rc.csizes, rc.offsets):
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        cs, of, packed = result(torch, rc, k)
        eager.compress_arrays(d_src, k)
        ecs, eof, epacked = result(torch, eager, k)
        assert (cs == ecs).all() and (of == eof).all() and packed.tobytes() == epacked.tobytes()
        assert int(cs[1]) == 9 and int(cs.min()) > 0
        seen.append(packed.tobytes())
    assert seen[0] != seen[1]


# ---- 7. the Python class -------------------------------------------------------------------------------------------
def test_python_class(torch_cuda):
    for kw in (dict(level=1), dict(level=3, compact=True),
               dict(level=3, dictionary=torch_cuda.zeros(64, dtype=torch_cuda.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            L.RaggedCodec("zstd_dfast", 65536, 4, **kw)
    rc = L.RaggedCodec("zstd_dfast", 65536, 4, level=3, compact_scratch=True, split_decode=True)
    lib = L.lib()
    assert rc.ctemp.numel() == lib.lzh_zstd_dfast_ragged_compact_compress_temp_bytes(3, 4 * 65536, 65536, 4)
    assert rc.dtemp.numel() == lib.lzh_zstd_ragged_decompress_split_temp_bytes(65536, 4)
    assert rc.max_packed == lib.lzh_zstd_ragged_max_packed_bytes(4 * 65536, 4)
