"""GPU: the compact compress layout of ragged batches (include/lzbench_hip.h 3b, RaggedCodec(compact=True)) --
every chunk's slots sized from its own size: against the CPU oracle, against the uniform-slot call byte for
byte, with the temp buffer at exactly the sizing answer and a guard after it, and with a broken promise.
Run with -m gpu."""
import numpy as np
import pytest

import lzbench_amd as L
from gpu_batches import check_batch, layout, roundtrip, to_dev, torch_cuda
from ragged_inputs import CASES, CASE_IDS, EDGE_SIZES, edge_input, expect, expected, raw_chunk

pytestmark = pytest.mark.gpu

GUARD = 4096


def compact_codec(torch, codec, level, maxb, k, total):
    """RaggedCodec(compact=True) whose temp is exactly the sizing answer, followed by a guard of 0xEE bytes that is
    not counted in temp_bytes."""
    rc = L.RaggedCodec(codec, maxb, k, level, max_total_bytes=total, compact=True)
    ct = L.lib().lzh_ragged_compact_compress_temp_bytes(rc.codec, total, maxb, k)
    assert rc.ctemp.numel() == ct
    buf = torch.full((ct + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.ctemp = buf[:ct]
    return rc, buf[ct:]


def guard_intact(torch, guard):
    torch.cuda.synchronize()
    return bool((guard == 0xEE).all())


def same_outputs(torch, a, b, k):
    torch.cuda.synchronize()
    assert torch.equal(a.csizes[:k], b.csizes[:k]), "csizes differ"
    assert torch.equal(a.offsets[: k + 1], b.offsets[: k + 1]), "offsets differ"
    total = b.packed_total()
    assert a.packed_total() == total and torch.equal(a.packed[:total], b.packed[:total]), "packed bytes differ"


@pytest.mark.parametrize("codec,level", CASES, ids=CASE_IDS)
def test_edge_sizes_in_one_batch(torch_cuda, edge_input, codec, level):
    torch = torch_cuda
    host, offs = edge_input
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    k = len(EDGE_SIZES)
    rc, guard = compact_codec(torch, codec, level, max(EDGE_SIZES), k, sum(EDGE_SIZES))
    d_in = to_dev(torch, host)
    rc.compress(d_in, offs, EDGE_SIZES)
    check_batch(torch, rc, len(EDGE_SIZES), expected(host, offs, EDGE_SIZES, codec, level))
    assert guard_intact(torch, guard)
    roundtrip(torch, rc, host, offs, EDGE_SIZES)
    # the uniform-slot call on the same arrays
    ru = L.RaggedCodec(codec, max(EDGE_SIZES), k, level, max_total_bytes=sum(EDGE_SIZES))
    ru.compress_arrays(rc._in, k)
    same_outputs(torch, rc, ru, k)


@pytest.mark.parametrize("codec,level", CASES, ids=CASE_IDS)
def test_equals_the_uniform_slot_call_on_many_small_chunks(torch_cuda, codec, level):
    torch = torch_cuda
    sizes = [int(s) for s in np.random.default_rng(31).integers(0, 5001, 300)]
    offs, total = layout(sizes, gap=1)
    host = L.datagen("mixed", total, seed=37)
    rc, guard = compact_codec(torch, codec, level, 5000, 300, sum(sizes))
    rc.compress(to_dev(torch, host), offs, sizes)
    check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level))
    ru = L.RaggedCodec(codec, 5000, 300, level, max_total_bytes=sum(sizes))
    ru.compress_arrays(rc._in, 300)
    same_outputs(torch, rc, ru, 300)
    assert guard_intact(torch, guard)


BIG = (1 << 20) + 3


@pytest.fixture(scope="module")
def skewed_input():
    """200 chunks of 1..5000 bytes and one chunk of 1 MiB + 3 that the test puts among them.  The big chunk's bytes
    are the same wherever it sits (the oracle's answer for it is computed once per case)."""
    small = [int(s) for s in np.random.default_rng(41).integers(1, 5001, 200)]
    big = L.datagen("text", BIG, seed=43)
    smalls = L.datagen("mixed", sum(small), seed=47)
    return small, big, smalls


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("codec,level", CASES, ids=CASE_IDS)
def test_a_skewed_batch(torch_cuda, skewed_input, codec, level, where):
    torch = torch_cuda
    small, big, smalls = skewed_input
    at = {"first": 0, "middle": 100, "last": 200}[where]
    sizes = small[:at] + [BIG] + small[at:]
    offs, total = layout(sizes)
    host = np.zeros(total, np.uint8)
    pos = 0
    for i, (o, s) in enumerate(zip(offs, sizes)):
        if i == at:
            host[o: o + s] = big
        else:
            host[o: o + s] = smalls[pos: pos + s]
            pos += s
    k = len(sizes)
    rc, guard = compact_codec(torch, codec, level, BIG, k, sum(sizes))
    # the point of the layout: this batch's temp is a fraction of the uniform slots'
    assert rc.ctemp.numel() * 20 < L.lib().lzh_ragged_compress_temp_bytes(rc.codec, BIG, k)
    rc.compress(to_dev(torch, host), offs, sizes)
    check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level))
    assert guard_intact(torch, guard), "write past the sizing answer"
    roundtrip(torch, rc, host, offs, sizes)


def raw_chunk_at(codec, level):
    """raw_chunk for every case: at acceleration 7 LZ4 steps over the 37-byte tail run of raw_chunk("lz4") (4114
    bytes, all literals); a run of 29 bytes at 100..128 of the same random bytes gives 4096 there (a CPU search over
    the oracle, as for the other two; the test asserts it)."""
    if codec == "lz4fast" and level == 7:
        d = L.datagen("random", 4096, seed=1).copy()
        d[100:129] = 0x42
        return d
    return raw_chunk(codec)


@pytest.mark.parametrize("codec,level", CASES, ids=CASE_IDS)
def test_incompressible_input_and_the_raw_store_rule(torch_cuda, codec, level):
    torch = torch_cuda
    parts = [L.datagen("text", 5000, seed=8), raw_chunk_at(codec, level), L.datagen("random", 65536, seed=2),
             L.datagen("text", 777, seed=9), L.datagen("random", 200000, seed=4), L.datagen("random", 4099, seed=6)]
    sizes = [len(p) for p in parts]
    offs, total = layout(sizes)
    host = np.zeros(total, np.uint8)
    for o, p in zip(offs, parts):
        host[o: o + len(p)] = p
    assert expect(parts[1], codec, level) == parts[1].tobytes()
    rc, guard = compact_codec(torch, codec, level, 200000, len(sizes), sum(sizes))
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, packed = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level))
    assert int(cs[1]) == 4096 and packed[of[1]: of[2]].tobytes() == parts[1].tobytes()   # stored raw: a copy
    for i in (2, 4, 5):   # random bytes expand: the staging slot is used to the codec's bound
        assert int(cs[i]) > sizes[i]
    assert guard_intact(torch, guard)
    roundtrip(torch, rc, host, offs, sizes)
    ru = L.RaggedCodec(codec, 200000, len(sizes), level)
    ru.compress_arrays(rc._in, len(sizes))
    same_outputs(torch, rc, ru, len(sizes))


@pytest.mark.parametrize("codec,level", CASES, ids=CASE_IDS)
def test_a_broken_promise(torch_cuda, edge_input, codec, level):
    """total_in_bytes at half the true sum: the chunks the host mirror marks processed match the oracle, the others
    take no bytes, nothing is written past the temp buffer or the packed buffer."""
    torch = torch_cuda
    host, offs = edge_input
    k, maxb = len(EDGE_SIZES), max(EDGE_SIZES)
    promised = sum(EDGE_SIZES) // 2
    rc, guard = compact_codec(torch, codec, level, maxb, k, promised)
    cap = rc.max_packed
    pbuf = torch.full((cap + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rc.packed = pbuf[:cap]
    szs = np.array(EDGE_SIZES, np.uint64)
    so, ro, pr = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.uint8)
    assert L.lib().lzh_debug_ragged_compact_slots(rc.codec, szs.ctypes.data, k, maxb, promised, so.ctypes.data,
                                                  ro.ctypes.data, pr.ctypes.data) == 0
    dropped = {i for i in range(k) if not pr[i]}
    assert dropped and len(dropped) < k
    d_in = to_dev(torch, host)
    both = np.stack([offs + d_in.data_ptr(), np.array(EDGE_SIZES, np.int64)])
    rc.compress_arrays(torch.from_numpy(both).cuda(), k)      # (compress() refuses the batch on the host)
    cs, of, _ = check_batch(torch, rc, len(EDGE_SIZES), expected(host, offs, EDGE_SIZES, codec, level), skip=dropped)
    for i in dropped:
        assert int(cs[i]) == 0 and of[i] == of[i + 1]
    assert guard_intact(torch, guard), "write past the temp buffer"
    assert int(of[k]) <= cap and bool((pbuf[int(of[k]):] == 0x5A).all()), "write past the packed total"


@pytest.mark.parametrize("codec,level", CASES, ids=CASE_IDS)
def test_oversize_chunk_is_not_processed(torch_cuda, codec, level):
    torch = torch_cuda
    maxb = 70000
    sizes = [3000, maxb + 1, maxb, 17]          # entry 1 is one byte too large (and really that large)
    offs, total = layout(sizes)
    host = L.datagen("text", total, seed=17)
    good = sum(sizes) - (maxb + 1)              # the promise covers the chunks that are not oversize
    rc, guard = compact_codec(torch, codec, level, maxb, len(sizes), good)
    cap = rc.max_packed
    pbuf = torch.full((cap + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rc.packed = pbuf[GUARD: GUARD + cap]
    d_in = to_dev(torch, host)
    both = np.stack([offs + d_in.data_ptr(), np.array(sizes, np.int64)])
    rc.compress_arrays(torch.from_numpy(both).cuda(), len(sizes))
    cs, of, _ = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level), skip={1})
    assert int(cs[1]) == 0 and of[1] == of[2]
    assert guard_intact(torch, guard), "write past the temp buffer"
    assert bool((pbuf[:GUARD] == 0x5A).all()) and bool((pbuf[GUARD + int(of[4]):] == 0x5A).all()), "write outside packed"
    rc.max_total = sum(sizes)   # (the host-side check of decompress() counts the oversize entry)
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})
    assert int(st[1]) == -1


@pytest.mark.parametrize("codec,level", CASES, ids=CASE_IDS)
def test_graph_replay_with_new_data(torch_cuda, codec, level):
    torch = torch_cuda
    sizes = [70000, 0, 13, 4099, 65536, 9]
    offs, total = layout(sizes)
    hosts = [L.datagen("json", total, seed=29), L.datagen("text", total, seed=53), L.datagen("mixed", total, seed=59)]
    d_in = to_dev(torch, hosts[0])
    rc = L.RaggedCodec(codec, 70000, len(sizes), level, max_total_bytes=sum(sizes), compact=True)
    d_src, k = rc._arrays(d_in, offs, sizes, 16)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rc.compress_arrays(d_src, k)
    check_batch(torch, rc, len(sizes), expected(hosts[0], offs, sizes, codec, level))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc.compress_arrays(d_src, k)
    for host in hosts[1:]:                       # the same buffers, other bytes in them
        d_in[: len(host)].copy_(torch.from_numpy(host))
        for t in (rc.packed, rc.csizes, rc.offsets):
            t.zero_()
        g.replay()
        check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level))
