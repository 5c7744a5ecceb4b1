"""GPU: the compact compress layout of ragged zstd batches (include/lzbench_hip.h 3c,
lzbench_amd.RaggedCodec("zstd", compact_scratch=True)) -- every chunk's staging slot and scratch slot sized from
its own size: the frames against the CPU restatement and the reference build, against the uniform-slot ragged
call and the uniform call, the placement on the device against its host mirror, and the guards.
Run with -m gpu."""
import numpy as np
import pytest

import lzbench_amd as L
from gpu_batches import SLACK, check_batch, layout, roundtrip, to_dev, torch_cuda
from zstd_ragged_inputs import EDGE_L2, EDGE_SIZES, codec_name, corpus_mix, edge_input, expected

pytestmark = pytest.mark.gpu

ZSTD = L.LZH_CODEC_ZSTD
G = 4096          # canary bytes on each side of a buffer


def a256(v):
    return (v + 255) // 256 * 256


def compact_codec(level, maxb, k, total):
    return L.RaggedCodec(codec_name(level), maxb, k, level, max_total_bytes=total, compact_scratch=True)


def with_canary(torch, rc):
    """rc's compress temp (exactly the sizing answer) and packed buffer inside larger tensors filled with 0xEE"""
    ct, mp = rc.ctemp.numel(), rc.packed.numel()
    temp = torch.full((ct + 2 * G,), 0xEE, dtype=torch.uint8, device="cuda")
    packed = torch.full((mp + 2 * G,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.ctemp, rc.packed = temp[G: G + ct], packed[G: G + mp]
    return temp, packed


def canary_intact(temp, packed, rc, packed_total):
    ct, mp = rc.ctemp.numel(), rc.packed.numel()
    assert bool((temp[:G] == 0xEE).all()) and bool((temp[G + ct:] == 0xEE).all()), "write outside the temp buffer"
    assert bool((packed[:G] == 0xEE).all()) and bool((packed[G + mp:] == 0xEE).all()), "write outside packed"
    assert bool((packed[G + packed_total: G + mp] == 0xEE).all()), "write past the packed total"


def mirror(level, sizes, maxb, total):
    s = np.ascontiguousarray(sizes, dtype=np.uint64)
    k = len(s)
    so, co, pr = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.uint8)
    assert L.lib().lzh_debug_zstd_ragged_compact_slots(level, s.ctypes.data, k, maxb, total, so.ctypes.data,
                                                       co.ctypes.data, pr.ctypes.data) == 0
    return so.astype(np.int64), co.astype(np.int64), pr.astype(bool)


def device_placement(rc, k):
    """the four per-chunk arrays at the end of the compress temp (temp_layout.h zstd_compact_temp), k = the
    codec's max_chunks: (staging-slot sizes, scratch-slot sizes, staging offsets, scratch offsets) of a batch"""
    t = rc.ctemp.cpu().numpy()
    a = len(t) - (2 * a256(4 * k) + 2 * a256(8 * (k + 1)))
    ssz = t[a: a + 4 * k].view(np.uint32).astype(np.int64)
    a += a256(4 * k)
    csz = t[a: a + 4 * k].view(np.uint32).astype(np.int64)
    a += a256(4 * k)
    sof = t[a: a + 8 * (k + 1)].view(np.uint64).astype(np.int64)
    a += a256(8 * (k + 1))
    cof = t[a: a + 8 * (k + 1)].view(np.uint64).astype(np.int64)
    return ssz, csz, sof, cof


# ---- 1. edge sizes in one batch: the reference frames, the uniform-slot call's outputs, the round trip --------
@pytest.mark.parametrize("level", [1, -1, -5, 2])
def test_edge_sizes_equal_the_uniform_slot_call(torch_cuda, edge_input, level):
    torch = torch_cuda
    host, offs = edge_input
    sizes = EDGE_L2 if level == 2 else EDGE_SIZES
    offs = offs[: len(sizes)]
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    k = len(sizes)
    d_in = to_dev(torch, host)
    rc = compact_codec(level, max(sizes), k, sum(sizes))
    rc.compress(d_in, offs, sizes)
    cs, of, packed = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level))
    assert int(cs[0]) == 9 and [int(c) for c in cs[1:4]] == [1 + 9, 6 + 9, 7 + 9]
    ru = L.RaggedCodec(codec_name(level), max(sizes), k, level, max_total_bytes=sum(sizes))
    ru.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    assert torch.equal(rc.csizes[:k], ru.csizes[:k]) and torch.equal(rc.offsets[: k + 1], ru.offsets[: k + 1])
    total = ru.packed_total()
    assert rc.packed_total() == total and torch.equal(rc.packed[:total], ru.packed[:total])
    # the placement on the device is the host mirror's
    so, co, pr = mirror(level, sizes, max(sizes), sum(sizes))
    ssz, csz, sof, cof = device_placement(rc, k)
    assert pr.all() and (sof[:k] == so).all() and (cof[:k] == co).all()
    assert (np.diff(sof) == ssz).all() and (np.diff(cof) == csz).all()
    roundtrip(torch, rc, host, offs, sizes)


# ---- 2. a skewed batch on the compact temp alone ---------------------------------------------------------------
# One chunk of 1 MiB (eight blocks) among small ones.  The tenth of the uniform-slot answer is asserted where the
# three numbers the sizing function sees admit it: 64 chunks within 1.25 MiB may also be 64 chunks of 16 KiB, and
# at level 1 such a chunk's hash table alone is 128 KiB (hashLog 15) -- 64 x (137 KiB of areas + 128 KiB of table
# + 17 KiB of staging) = 18 MB, over a tenth of the 152 MB of the uniform slots, for any correct sizing.  At the
# negative levels the table is 32 KiB and 64 chunks do; level 1 takes 256 chunks.
@pytest.mark.parametrize("level,k", [(-1, 64), (-5, 64), (1, 256)])
def test_skewed_batch(torch_cuda, level, k):
    torch = torch_cuda
    maxb = 1 << 20
    rng = np.random.default_rng(100 + level)
    sizes = [int(s) for s in rng.integers(0, 4097, k)]
    sizes[0], sizes[1], sizes[2], sizes[5] = 0, 7, 4096, maxb
    offs, total = layout(sizes)
    host = corpus_mix(total, 50 + level)
    rc = compact_codec(level, maxb, k, sum(sizes))
    uniform = L.lib().lzh_zstd_ragged_compress_temp_bytes(level, maxb, k)
    print(f"level {level}, {k} chunks, {sum(sizes)} bytes: compact temp {rc.ctemp.numel()}, uniform slots {uniform}")
    assert rc.ctemp.numel() * 10 < uniform
    temp, packed = with_canary(torch, rc)
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, _ = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level))
    canary_intact(temp, packed, rc, int(of[k]))
    roundtrip(torch, rc, host, offs, sizes)


# ---- 3. temp guard: a chunk over max_chunk_bytes -----------------------------------------------------------------
@pytest.mark.parametrize("level", [1, -1])
def test_oversize_chunk_and_temp_guard(torch_cuda, level):
    torch = torch_cuda
    maxb = 140000                               # (two blocks: the second launch pair must skip the chunk as well)
    sizes = [3000, maxb + 1, maxb, 17, 0]       # entry 1 is one byte too large (and really that large)
    k = len(sizes)
    offs, total = layout(sizes)
    host = corpus_mix(total, 17)
    promise = sum(s for s in sizes if s <= maxb)
    rc = compact_codec(level, maxb, k, sum(sizes))
    rc.max_total = promise                      # (the promise leaves the oversize chunk out; buffers as built)
    ct = L.lib().lzh_zstd_ragged_compact_compress_temp_bytes(level, promise, maxb, k)
    rc.ctemp = rc.ctemp[:ct]
    temp, packed = with_canary(torch, rc)
    d_in = to_dev(torch, host)
    d = torch.from_numpy(np.stack([offs + d_in.data_ptr(), np.array(sizes, np.int64)])).cuda()
    rc.compress_arrays(d, k)
    cs, of, _ = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level), skip={1})
    assert int(cs[1]) == 0 and of[1] == of[2]
    canary_intact(temp, packed, rc, int(of[k]))
    # the oversize chunk took slots of 0 bytes; its neighbours' slots are where the host mirror puts them
    so, co, pr = mirror(level, sizes, maxb, promise)
    ssz, csz, sof, cof = device_placement(rc, k)
    assert pr.tolist() == [True, False, True, True, True]
    assert ssz[1] == 0 and csz[1] == 0 and (sof[:k] == so).all() and (cof[:k] == co).all()
    rc.max_total = sum(sizes)                   # (the decode side's host check counts every entry)
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})
    assert int(st[1]) == -1


# ---- 4. a broken promise -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, -5])
def test_broken_promise_drops_exactly_the_chunks_the_mirror_names(torch_cuda, level):
    torch = torch_cuda
    sizes = [5000, 70000, 16384, 0, 300, 131073, 9000, 4099, 7, 40000]
    k, maxb = len(sizes), max(sizes)
    offs, total = layout(sizes)
    host = corpus_mix(total, 61)
    claim = sum(sizes) // 3                      # understated
    so, co, pr = mirror(level, sizes, maxb, claim)
    first = int(np.flatnonzero(~pr)[0])
    assert 2 <= first < k - 1 and not pr[first:].any() and pr[:first].all()    # the last chunks, and several of them
    rc = compact_codec(level, maxb, k, sum(sizes))   # (packed sized for the true total)
    rc.max_total = claim
    ct = L.lib().lzh_zstd_ragged_compact_compress_temp_bytes(level, claim, maxb, k)
    assert ct < rc.ctemp.numel()
    rc.ctemp = rc.ctemp[:ct]
    temp, packed = with_canary(torch, rc)
    d_in = to_dev(torch, host)
    d = torch.from_numpy(np.stack([offs + d_in.data_ptr(), np.array(sizes, np.int64)])).cuda()
    rc.compress_arrays(d, k)
    dropped = set(range(first, k))
    # (offsets: the scan; [k]: the sum)
    cs, of, _ = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level), skip=dropped)
    assert all(int(cs[i]) == 0 for i in dropped) and all(int(cs[i]) > 0 for i in range(first))
    assert int(of[k]) == int(cs.sum())
    canary_intact(temp, packed, rc, int(of[k]))
    ssz, csz, sof, cof = device_placement(rc, k)
    assert (sof[:k] == so).all() and (cof[:k] == co).all()


# ---- 5. equal sizes over contiguous input: the uniform call's bytes ----------------------------------------------
@pytest.mark.parametrize("level", [1, -1])
def test_equals_the_uniform_call(torch_cuda, level):
    torch = torch_cuda
    chunk, k = 65536, 16
    n = chunk * k
    host = corpus_mix(n, 3)
    d_in = to_dev(torch, host, SLACK)
    dc = L.DeviceCodec(codec_name(level), n, chunk, level)
    dc.compress(d_in)
    rc = compact_codec(level, chunk, k, n)
    rc.compress(d_in, np.arange(k, dtype=np.int64) * chunk, [chunk] * k)
    torch.cuda.synchronize()
    assert dc.k == k
    assert torch.equal(rc.csizes[:k], dc.csizes) and torch.equal(rc.offsets[: k + 1], dc.offsets)
    total = dc.packed_total()
    assert rc.packed_total() == total and torch.equal(rc.packed[:total], dc.packed[:total])


# ---- 6. one codec, two batches back to back ----------------------------------------------------------------------
def test_reuse_of_one_codec(torch_cuda):
    """the second batch's slots lie across the first one's (other sizes, other block counts): no state leaks
    through scratch headers, saved tables or staged bytes"""
    torch = torch_cuda
    level = 1
    first = [140000, 9, 131073, 4099, 70000, 0, 300000, 16384]
    second = [7, 300000, 0, 16385, 140000, 131072, 5, 65536, 255]
    maxb, k = 300000, 9
    rc = compact_codec(level, maxb, k, max(sum(first), sum(second)))
    for sizes, seed in ((first, 71), (second, 72)):
        offs, total = layout(sizes)
        host = corpus_mix(total, seed)
        rc.compress(to_dev(torch, host), offs, sizes)
        check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level))
    roundtrip(torch, rc, host, offs, sizes)
