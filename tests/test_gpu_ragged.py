"""GPU: ragged batches on the device API (include/lzbench_hip.h 3b, lzbench_amd.RaggedCodec) -- per-chunk
pointers and sizes against the CPU oracle chunk by chunk, against the uniform call, and their guards.
Run with -m gpu."""
import numpy as np
import pytest

import lzbench_amd as L
from gpu_batches import SLACK, check_batch, layout, roundtrip, to_dev, torch_cuda
from ragged_inputs import CASES, CASE_IDS, EDGE_SIZES, edge_input, expect, expected, raw_chunk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("codec,level", CASES, ids=CASE_IDS)
def test_edge_sizes_in_one_batch(torch_cuda, edge_input, codec, level):
    torch = torch_cuda
    host, offs = edge_input
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    rc = L.RaggedCodec(codec, max(EDGE_SIZES), len(EDGE_SIZES), level, max_total_bytes=sum(EDGE_SIZES))
    rc.compress(to_dev(torch, host), offs, EDGE_SIZES)
    check_batch(torch, rc, len(EDGE_SIZES), expected(host, offs, EDGE_SIZES, codec, level))
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
    cs, of, packed = check_batch(torch, rc, len(p_sizes), expected(host, p_offs, p_sizes, codec, level))
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
    cs, of, packed = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level))
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
    check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level))
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
    cs, of, _ = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level), skip={1})
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
    cs, of, packed = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level))
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
        check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level))
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
