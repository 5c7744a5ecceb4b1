"""GPU: ragged batches on the device API (include/lzbench_hip.h 3b, lzbench_amd.RaggedCodec) -- per-chunk
pointers and sizes against the CPU oracle chunk by chunk, against the uniform call, and their guards.
Run with -m gpu."""
import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L

pytestmark = pytest.mark.gpu

# (codec name, level): LZ4_compress_default, LZ4_compress_fast at acceleration 7, snappy
CASES = [("lz4", 1), ("lz4fast", 7), ("snappy", 0)]
CASE_IDS = ["lz4", "lz4-acc7", "snappy"]
# 65546 | 65547: LZ4's byU16 / byU32 tables; 14 | 15: snappy's all-literal bound; 200000: four snappy fragments
EDGE_SIZES = [70000, 0, 1, 12, 13, 14, 15, 16, 255, 4099, 65535, 65536, 65546, 65547, 200000, 3]
SLACK = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    return torch


_expect_cache = {}


def expect(chunk: np.ndarray, codec: str, level: int) -> bytes:
    """The packed bytes of one chunk from the CPU oracle (raw-store rule applied; cached), checked against the
    reference build's own functions where that is present."""
    key = (chunk.tobytes(), codec, level)
    if key not in _expect_cache:
        if len(chunk):
            packed, cs = O.compress_chunks(np.ascontiguousarray(chunk), codec, len(chunk), level)
            assert len(cs) == 1 and int(cs[0]) == len(packed)
        else:   # (the oracle's chunk loop has no chunk for an empty input: its block functions, one byte each)
            empty = np.zeros(1, np.uint8)[:0]
            packed = np.frombuffer(O.snappy_compress(empty) if codec == "snappy" else O.lz4_compress(empty, max(level, 1)),
                                   np.uint8)
            assert len(packed) == 1
        if O.have_ref():
            R = O.ref()
            src = np.ascontiguousarray(chunk) if len(chunk) else np.zeros(1, np.uint8)
            dst = np.zeros(len(chunk) + len(chunk) // 6 + 1024, np.uint8)
            if codec == "snappy":
                r = R.ref_snappy_compress(src.ctypes.data, len(chunk), dst.ctypes.data)
            else:   # (ref_lz4_compress_fast at acceleration 1 is LZ4_compress_default)
                r = R.ref_lz4_compress_fast(src.ctypes.data, dst.ctypes.data, len(chunk), len(dst), max(level, 1))
            ref = chunk.tobytes() if r == len(chunk) else dst[:r].tobytes()
            assert ref == packed.tobytes(), "oracle and reference build differ"
        _expect_cache[key] = packed.tobytes()
    return _expect_cache[key]


def layout(sizes, residues=(1, 2, 3, 0), gap=5):
    """Offsets for chunks of `sizes` in one flat buffer: gaps between chunks, pointers over all residues mod 4."""
    offs, pos = [], 0
    for i, s in enumerate(sizes):
        pos += gap
        pos += (residues[i % len(residues)] - pos) % 4
        offs.append(pos)
        pos += s
    return np.array(offs, np.int64), pos + SLACK


def to_dev(torch, a: np.ndarray, pad=0):
    t = torch.zeros(len(a) + pad, dtype=torch.uint8, device="cuda")
    t[: len(a)].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def check_batch(torch, rc, host, offs, sizes, codec, level, skip=()):
    """csizes, offsets and every packed byte range of rc's last compress call against the oracle."""
    torch.cuda.synchronize()
    k = len(sizes)
    cs = rc.csizes[:k].cpu().numpy().astype(np.int64)
    of = rc.offsets[: k + 1].cpu().numpy()
    assert (of == np.concatenate([[0], np.cumsum(cs)])).all(), "offsets are not the exclusive scan of csizes"
    assert rc.packed_total() == int(cs.sum())
    packed = rc.packed[: int(of[k])].cpu().numpy()
    for i in range(k):
        if i in skip:
            continue
        e = expect(host[offs[i]: offs[i] + sizes[i]], codec, level)
        assert int(cs[i]) == len(e), f"chunk {i} ({sizes[i]} bytes): csize {cs[i]}, oracle {len(e)}"
        assert packed[of[i]: of[i + 1]].tobytes() == e, f"chunk {i} ({sizes[i]} bytes): packed bytes differ"
    return cs, of, packed


def roundtrip(torch, rc, host, offs, sizes, skip=()):
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    rc.decompress(out, offs, sizes)
    torch.cuda.synchronize()
    st = rc.status[: len(sizes)].cpu().numpy()
    got = out.cpu().numpy()
    mask = np.zeros(len(host), bool)
    for i in range(len(sizes)):
        if i in skip:
            continue
        assert int(st[i]) == sizes[i], f"chunk {i}: status {st[i]}"
        assert (got[offs[i]: offs[i] + sizes[i]] == host[offs[i]: offs[i] + sizes[i]]).all(), f"chunk {i}: roundtrip"
        mask[offs[i]: offs[i] + sizes[i]] = True
    assert (got[~mask] == 0xEE).all(), "the decoder wrote outside the chunks"
    return st


@pytest.fixture(scope="module")
def edge_input():
    offs, total = layout(EDGE_SIZES)
    return L.datagen("text", total, seed=21), offs


@pytest.mark.parametrize("codec,level", CASES, ids=CASE_IDS)
def test_edge_sizes_in_one_batch(torch_cuda, edge_input, codec, level):
    torch = torch_cuda
    host, offs = edge_input
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    rc = L.RaggedCodec(codec, max(EDGE_SIZES), len(EDGE_SIZES), level, max_total_bytes=sum(EDGE_SIZES))
    rc.compress(to_dev(torch, host), offs, EDGE_SIZES)
    check_batch(torch, rc, host, offs, EDGE_SIZES, codec, level)
    roundtrip(torch, rc, host, offs, EDGE_SIZES)


@pytest.mark.parametrize("codec,level", [CASES[0], CASES[2]], ids=["lz4", "snappy"])
def test_order_and_aliasing(torch_cuda, edge_input, codec, level):
    torch = torch_cuda
    host, offs = edge_input
    perm = np.random.default_rng(5).permutation(len(EDGE_SIZES))
    p_offs = np.concatenate([offs[perm], offs[[0, 0, 9]]])          # two entries at chunk 0's bytes, a third at 9's
    p_sizes = [EDGE_SIZES[i] for i in perm] + [EDGE_SIZES[0], EDGE_SIZES[0], EDGE_SIZES[9]]
    rc = L.RaggedCodec(codec, max(EDGE_SIZES), len(p_sizes), level)
    rc.compress(to_dev(torch, host), p_offs, p_sizes)
    cs, of, packed = check_batch(torch, rc, host, p_offs, p_sizes, codec, level)
    k = len(p_sizes)
    assert packed[of[k - 3]: of[k - 2]].tobytes() == packed[of[k - 2]: of[k - 1]].tobytes()


@pytest.mark.parametrize("codec,level", [CASES[0], CASES[2]], ids=["lz4", "snappy"])
@pytest.mark.parametrize("chunk", [65536, 4099])
def test_equals_the_uniform_call(torch_cuda, codec, level, chunk):
    torch = torch_cuda
    n = 1 << 20
    host = L.datagen("text", n, seed=3)
    d_in = to_dev(torch, host, SLACK)
    dc = L.DeviceCodec(codec, n, chunk)
    dc.compress(d_in)
    sizes = L.chunk_sizes_for(n, chunk).astype(np.int64)
    offs = np.arange(len(sizes), dtype=np.int64) * chunk
    rc = L.RaggedCodec(codec, chunk, len(sizes), level, max_total_bytes=n)
    rc.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    k = len(sizes)
    assert dc.k == k
    assert torch.equal(rc.csizes[:k], dc.csizes) and torch.equal(rc.offsets[: k + 1], dc.offsets)
    total = dc.packed_total()
    assert rc.packed_total() == total and torch.equal(rc.packed[:total], dc.packed[:total])


def raw_chunk(codec):
    """4096 bytes whose compressed size is 4096 (found by a CPU search over the oracle: random bytes of seed 1
    with one short run; LZ4: the last 37 bytes, snappy: bytes 100..114)."""
    d = L.datagen("random", 4096, seed=1).copy()
    if codec == "snappy":
        d[100:115] = 0x42
    else:
        d[4096 - 37:] = 0x41
    return d


@pytest.mark.parametrize("codec,level", [CASES[0], CASES[2]], ids=["lz4", "snappy"])
def test_raw_store_rule(torch_cuda, codec, level):
    torch = torch_cuda
    parts = [L.datagen("text", 5000, seed=8), raw_chunk(codec), L.datagen("random", 65536, seed=2),
             L.datagen("text", 777, seed=9), L.datagen("random", 65536, seed=4)]
    sizes = [len(p) for p in parts]
    offs, total = layout(sizes)
    host = np.zeros(total, np.uint8)
    for o, p in zip(offs, parts):
        host[o: o + len(p)] = p
    assert len(expect(parts[1], codec, level)) == 4096 and expect(parts[1], codec, level) == parts[1].tobytes()
    rc = L.RaggedCodec(codec, 65536, len(sizes), level)
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, packed = check_batch(torch, rc, host, offs, sizes, codec, level)
    assert int(cs[1]) == 4096 and packed[of[1]: of[2]].tobytes() == parts[1].tobytes()   # stored raw: a copy
    roundtrip(torch, rc, host, offs, sizes)


@pytest.mark.parametrize("codec,level", [CASES[0], CASES[2]], ids=["lz4", "snappy"])
def test_many_chunks(torch_cuda, codec, level):
    torch = torch_cuda
    sizes = [int(s) for s in np.random.default_rng(11).integers(0, 9001, 1000)]
    offs, total = layout(sizes, gap=1)
    host = L.datagen("mixed", total, seed=13)
    rc = L.RaggedCodec(codec, 9000, 1000, level, max_total_bytes=sum(sizes))
    rc.compress(to_dev(torch, host), offs, sizes)
    check_batch(torch, rc, host, offs, sizes, codec, level)
    roundtrip(torch, rc, host, offs, sizes)


@pytest.mark.parametrize("codec,level", [CASES[0], CASES[2]], ids=["lz4", "snappy"])
def test_oversize_chunk_is_not_processed(torch_cuda, codec, level):
    torch = torch_cuda
    maxb = 70000
    sizes = [3000, maxb + 1, maxb, 17]          # entry 1 is one byte too large (and really that large)
    offs, total = layout(sizes)
    host = L.datagen("text", total, seed=17)
    rc = L.RaggedCodec(codec, maxb, len(sizes), level, max_total_bytes=sum(sizes))
    # canaries: the temp buffer and the packed buffer get 4096 guard bytes on both sides
    G = 4096
    lib = L.lib()
    ct = lib.lzh_ragged_compress_temp_bytes(rc.codec, maxb, len(sizes))
    temp = torch.full((ct + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    packed = torch.full((rc.max_packed + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    rc.ctemp, rc.packed = temp[G: G + ct], packed[G: G + rc.max_packed]
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, _ = check_batch(torch, rc, host, offs, sizes, codec, level, skip={1})
    assert int(cs[1]) == 0 and of[1] == of[2]
    assert bool((temp[:G] == 0xA5).all()) and bool((temp[G + ct:] == 0xA5).all()), "write outside the temp buffer"
    assert bool((packed[:G] == 0x5A).all()) and bool((packed[G + int(of[4]):] == 0x5A).all()), "write outside packed"
    # the oversize chunk's staging slot (slot 1) was not touched
    stride = lib.lzh_stage_stride(rc.codec, maxb)
    assert bool((temp[G + stride: G + 2 * stride] == 0xA5).all()), "the oversize chunk's staging slot was written"
    # decode side: the same entry reports -1 and writes nothing; its neighbours decode
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})
    assert int(st[1]) == -1


@pytest.mark.parametrize("codec,level", [CASES[0], CASES[2]], ids=["lz4", "snappy"])
def test_malformed_chunks_get_the_uniform_verdicts(torch_cuda, codec, level):
    torch = torch_cuda
    sizes = [4099, 30000, 65536, 12000, 255]
    offs, total = layout(sizes)
    host = L.datagen("text", total, seed=23)
    rc = L.RaggedCodec(codec, 65536, len(sizes), level)
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, packed = check_batch(torch, rc, host, offs, sizes, codec, level)
    # corruptions of tests/test_gpu_fuzz.py: chunk 1 truncated by one byte, one bit flipped early in chunk 3
    bad_cs = cs.copy()
    bad_cs[1] -= 1
    bad = packed.copy()
    bad[of[3] + 9] ^= 0x10
    d_bad = to_dev(torch, bad, 256)
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    rc.decompress(out, offs, sizes, packed=d_bad, csizes=torch.from_numpy(bad_cs.astype(np.int32)).cuda(),
                  offsets=rc.offsets)
    torch.cuda.synchronize()
    st = rc.status[: len(sizes)].cpu().numpy()
    got = out.cpu().numpy()
    for i in (1, 3):   # the same block as a one-chunk batch of the uniform call
        block = bad[of[i]: of[i] + bad_cs[i]]
        dc = L.DeviceCodec(codec, sizes[i], sizes[i])
        dc.decompress(packed=to_dev(torch, block, 256), csizes=torch.tensor([len(block)], dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert int(st[i]) == int(dc.status[0].item()), f"chunk {i}: ragged {st[i]}, uniform {int(dc.status[0].item())}"
    for i in (0, 2, 4):
        assert int(st[i]) == sizes[i]
        assert (got[offs[i]: offs[i] + sizes[i]] == host[offs[i]: offs[i] + sizes[i]]).all()


@pytest.mark.parametrize("codec,level", [CASES[0], CASES[2]], ids=["lz4", "snappy"])
def test_side_stream_and_graph_replay(torch_cuda, codec, level):
    torch = torch_cuda
    sizes = [70000, 0, 13, 4099, 65536, 9]
    offs, total = layout(sizes)
    host = L.datagen("json", total, seed=29)
    d_in = to_dev(torch, host)
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    rc = L.RaggedCodec(codec, 70000, len(sizes), level)
    d_src, k = rc._arrays(d_in, offs, sizes, 16)
    d_dst, _ = rc._arrays(out, offs, sizes, 0)
    torch.cuda.synchronize()

    def pair():
        rc.compress_arrays(d_src, k)
        rc.decompress_arrays(d_dst, k)

    def check():
        torch.cuda.synchronize()
        check_batch(torch, rc, host, offs, sizes, codec, level)
        got = out.cpu().numpy()
        assert (rc.status[:k].cpu().numpy() == np.array(sizes)).all()
        for o, s in zip(offs, sizes):
            assert (got[o: o + s] == host[o: o + s]).all()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair()                                   # no host synchronisation between the two calls
    check()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair()
    for t in (out, rc.packed, rc.csizes, rc.offsets, rc.status):
        t.zero_()
    g.replay()
    check()
