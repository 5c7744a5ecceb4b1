"""CPU: the compact compress layout of ragged batches (include/lzbench_hip.h 3b) without a device -- the sizing
function and the host mirror of the slot placement against the regions the sizing answer holds."""
import numpy as np
import pytest

import lzbench_amd as L

LZ4, SNAPPY = L.LZH_CODEC_LZ4, L.LZH_CODEC_SNAPPY
OTHERS = (L.LZH_CODEC_MEMCPY, L.LZH_CODEC_ZSTD, L.LZH_CODEC_LZ4F, L.LZH_CODEC_NVLZ4)
OK, EARG = 0, -1
MAXB = 16 << 20


def test_symbols_exist():
    lib = L.lib()
    for name in ("lzh_ragged_compact_compress_temp_bytes", "lzh_compress_ragged_compact_async",
                 "lzh_debug_ragged_compact_slots", "lzh_debug_ragged_compact_regions"):
        assert hasattr(lib, name) and name in L.SIGNATURES


def sizing(codec, total, maxb, k):
    return L.lib().lzh_ragged_compact_compress_temp_bytes(codec, total, maxb, k)


def test_sizing_unsupported():
    for codec in OTHERS:
        assert sizing(codec, 1 << 20, 65536, 16) == 0
    for codec in (LZ4, SNAPPY):
        assert sizing(codec, 1 << 20, MAXB + 1, 16) == 0
        assert sizing(codec, 1 << 20, MAXB, 16) > 0
        assert sizing(codec, 0, 0, 0) > 0


@pytest.mark.parametrize("codec", [LZ4, SNAPPY])
def test_sizing_is_monotone(codec):
    totals = (0, 1, 254, 255, 256, 4099, 65535, 65536, 65537, 1 << 20, (1 << 20) + 1, 1 << 30, 1 << 36)
    maxbs = (0, 1, 15, 4099, 65535, 65536, 65537, 131072, 131073, 1 << 20, MAXB)
    ks = (0, 1, 2, 255, 256, 257, 1000, 16384, 1 << 20)
    for maxb in maxbs:
        for k in ks:
            v = [sizing(codec, t, maxb, k) for t in totals]
            assert all(a <= b for a, b in zip(v, v[1:])) and v[0] > 0, ("total", maxb, k)
    for t in totals:
        for k in ks:
            v = [sizing(codec, t, m, k) for m in maxbs]
            assert all(a <= b for a, b in zip(v, v[1:])), ("max_chunk_bytes", t, k)
        for maxb in maxbs:
            v = [sizing(codec, t, maxb, k) for k in ks]
            assert all(a <= b for a, b in zip(v, v[1:])), ("nchunks", t, maxb)


@pytest.mark.parametrize("codec", [LZ4, SNAPPY])
def test_skewed_batch_sizes_to_a_fraction_of_the_uniform_slots(codec):
    """4096 chunks, one of 16 MiB and 4095 of 4 KiB: about 32 MiB of input."""
    k, total = 4096, MAXB + 4095 * 4096
    compact = sizing(codec, total, MAXB, k)
    uniform = L.lib().lzh_ragged_compress_temp_bytes(codec, MAXB, k)
    assert 0 < compact * 100 < uniform, (compact, uniform)
    # and it is what the text says it is: the staging and record bytes of the total, a constant per chunk
    assert compact < 3.3 * total + k * (2048 + 4 * 256)


def mirror(codec, sizes, maxb, total):
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    k = len(sizes)
    so, ro, pr = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.uint8)
    rc = L.lib().lzh_debug_ragged_compact_slots(codec, sizes.ctypes.data, k, maxb, total, so.ctypes.data, ro.ctypes.data,
                                                pr.ctypes.data)
    assert rc == OK
    return so.astype(np.int64), ro.astype(np.int64), pr.astype(bool)


def slot_bytes(codec, n, maxb):
    """The slots of a chunk of n bytes as the existing sizing functions give them (n <= maxb), written out
    independently of csrc/ragged_slots.h: the staging slot is the uniform call's stride for that size; the
    record slot is 8 bytes per 4 input bytes and a few more, and in a snappy batch with more than one 64 KiB
    fragment per chunk, fragment f's records start at record f * (16384 + 32)."""
    lib = L.lib()
    st = lib.lzh_stage_stride(codec, n)
    a256 = lambda v: (v + 255) // 256 * 256
    if codec == LZ4:
        rec = a256((n // 4 + 4) * 8)
    elif maxb <= 65536:
        rec = a256((n // 4 + 8) * 8)
    elif n == 0:
        rec = 0
    else:
        nf = (n + 65535) // 65536
        rec = (nf - 1) * (16384 + 32) * 8 + a256(((n - (nf - 1) * 65536) // 4 + 8) * 8)
    return st, rec


def regions(codec, total, maxb, k):
    """(staging offset, staging bytes, record offset, record bytes) inside the temp buffer, checked against the
    sizing answer: inside it, disjoint, 256-aligned."""
    out = np.zeros(4, np.uint64)
    assert L.lib().lzh_debug_ragged_compact_regions(codec, total, maxb, k, out.ctypes.data) == OK
    s0, sb, r0, rb = (int(v) for v in out)
    ans = sizing(codec, total, maxb, k)
    assert s0 % 256 == 0 and r0 % 256 == 0
    assert s0 + sb <= r0 and r0 + rb <= ans, (s0, sb, r0, rb, ans)
    return s0, sb, r0, rb


def random_lists(rng, maxb, count):
    """Size lists of 1..40 chunks: the sizes around the 64 KiB fragment, small ones with a few large ones, all at
    the largest size, and sizes whose remainders cost the most alignment."""
    edge = [0, 1, 2, 3, 4, 15, 16, 255, 256, 4095, 4096, 65535, 65536, 65537, 65538, 131071, 131072, 131073]
    for it in range(count):
        k = int(rng.integers(1, 40))
        kind = it % 4
        if kind == 0:
            s = rng.choice([e for e in edge if e <= maxb], k)
        elif kind == 1:
            s = rng.integers(0, min(maxb, 5000) + 1, k)
            for j in rng.choice(k, min(k, 3), replace=False):
                s[j] = int(rng.integers(0, maxb + 1))
        elif kind == 2:
            s = np.full(k, maxb)
        else:
            s = np.minimum(maxb, rng.integers(0, 300, k) * 256 + rng.choice([0, 1, 253, 254, 255], k))
        yield np.asarray(s, np.int64)


def slots(codec, sizes, maxb):
    st, rec = zip(*(slot_bytes(codec, int(n), maxb) if n <= maxb else (0, 0) for n in sizes))
    return np.array(st, np.int64), np.array(rec, np.int64)


@pytest.mark.parametrize("codec", [LZ4, SNAPPY])
@pytest.mark.parametrize("maxb", [4096, 65536, 65537, 1 << 20, MAXB])
def test_a_kept_promise_places_every_slot_inside_its_region(codec, maxb):
    rng = np.random.default_rng(maxb + codec)
    for sizes in random_lists(rng, maxb, 100):
        k, true_total = len(sizes), int(sizes.sum())
        # the promise spent to the last byte, a loose one, and buffers sized for more chunks than the batch has
        for total, pad in ((true_total, 0), (true_total + int(rng.integers(0, 1 << 20)), 0), (true_total, 7)):
            szs = np.concatenate([sizes, np.zeros(pad, np.int64)])
            so, ro, pr = mirror(codec, szs, maxb, total)
            assert pr.all(), (szs, total)
            st, rec = slots(codec, szs, maxb)
            _, sb, _, rb = regions(codec, total, maxb, len(szs))
            assert (so % 256 == 0).all() and (ro % 256 == 0).all()
            assert so[0] >= 0 and ro[0] >= 0
            assert (so[1:] >= so[:-1] + st[:-1]).all() and (ro[1:] >= ro[:-1] + rec[:-1]).all(), "slots overlap"
            assert int((so + st).max()) <= sb and int((ro + rec).max()) <= rb, (szs, total)


@pytest.mark.parametrize("codec", [LZ4, SNAPPY])
@pytest.mark.parametrize("maxb", [4096, 65536, 1 << 20])
def test_a_broken_promise_drops_exactly_the_chunks_that_do_not_fit(codec, maxb):
    rng = np.random.default_rng(7 * maxb + codec)
    dropped = 0
    for sizes in random_lists(rng, maxb, 80):
        true_total = int(sizes.sum())
        if true_total < 2:
            continue
        for total in (true_total // 2, true_total // 8, 0):
            so, ro, pr = mirror(codec, sizes, maxb, total)
            st, rec = slots(codec, sizes, maxb)
            _, sb, _, rb = regions(codec, total, maxb, len(sizes))
            fits = (so + st <= sb) & (ro + rec <= rb)
            assert (pr == fits).all(), (sizes, total)
            assert (so[1:] >= so[:-1] + st[:-1]).all() and (ro[1:] >= ro[:-1] + rec[:-1]).all()
            dropped += int((~pr).sum())
    assert dropped > 0
    # a chunk over max_chunk_bytes takes no slot bytes and is not processed; its neighbours are
    sizes = np.array([100, maxb + 1, 200], np.int64)
    so, ro, pr = mirror(codec, sizes, maxb, 300)
    assert pr.tolist() == [True, False, True] and so[1] == so[2] and ro[1] == ro[2]


def test_the_slot_mirror_refuses_what_the_call_refuses():
    """(the call's own checks: tests/test_ragged_calls_abi.py)"""
    lib = L.lib()
    one = np.zeros(1, np.uint64)
    for codec, maxb in [(c, 65536) for c in OTHERS] + [(LZ4, MAXB + 1), (SNAPPY, MAXB + 1)]:
        assert lib.lzh_debug_ragged_compact_slots(codec, one.ctypes.data, 1, maxb, 0, one.ctypes.data, one.ctypes.data,
                                                  one.ctypes.data) == EARG


