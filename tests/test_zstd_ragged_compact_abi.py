"""CPU: the compact compress layout of ragged zstd batches (include/lzbench_hip.h 3c) without a device -- the
sizing function, the host mirror of the slot placement against the regions the sizing answer holds (the scratch
slots against an independent restatement of the zstd kernels' per-frame layout)."""
import numpy as np
import pytest

import lzbench_amd as L

ZSTD = L.LZH_CODEC_ZSTD
OK, EARG = 0, -1
MAX = 16 << 20
# (level, largest max_chunk_bytes it is accepted for)
GOOD = [(1, MAX), (2, 131072), (-1, MAX), (-5, MAX)]
FIXED = [0, 1, 6, 7, 8, 255, 1023, 1024, 4099, 16383, 16384, 16385, 65536, 131071, 131072, 131073, 262144, 262145,
         300000, MAX]


def test_symbols_exist():
    lib = L.lib()
    for name in ("lzh_zstd_ragged_compact_compress_temp_bytes", "lzh_zstd_compress_ragged_compact_async",
                 "lzh_debug_zstd_ragged_compact_slots", "lzh_debug_zstd_ragged_compact_regions"):
        assert hasattr(lib, name) and name in L.SIGNATURES


def sizing(level, total, maxb, k):
    return L.lib().lzh_zstd_ragged_compact_compress_temp_bytes(level, total, maxb, k)


def a256(v):
    return (v + 255) // 256 * 256


def arrays_bytes(k):
    """the four per-chunk arrays: two of k u32, two of k + 1 u64, each 256-aligned"""
    return 2 * a256(4 * k) + 2 * a256(8 * (k + 1))


# ---- the sizing function ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,maxb", [(3, 65536), (0, 65536), (19, 4096), (2, 131073), (2, 1 << 20), (1, MAX + 1),
                                        (-1, MAX + 1), (2, MAX + 1)])
def test_sizing_unsupported(level, maxb):
    assert sizing(level, 1 << 20, maxb, 16) == 0
    assert sizing(level, 0, maxb, 0) == 0


@pytest.mark.parametrize("level,top", GOOD)
def test_sizing_is_monotone(level, top):
    totals = (0, 1, 63, 64, 255, 256, 4099, 16384, 16385, 65536, 131073, 1 << 20, (1 << 20) + 1, 1 << 30, 1 << 36)
    maxbs = [m for m in (0, 1, 6, 7, 63, 64, 65, 1023, 1024, 4099, 16383, 16384, 16385, 16386, 32768, 65536, 131071,
                         131072, 131073, 262144, 262145, 300000, 1 << 20, MAX) if m <= top]
    ks = (0, 1, 2, 255, 256, 257, 1000, 16384, 1 << 20)
    for maxb in maxbs:
        for k in ks:
            v = [sizing(level, t, maxb, k) for t in totals]
            assert all(a <= b for a, b in zip(v, v[1:])) and v[0] > 0, ("total", maxb, k)
    for t in totals:
        for k in ks:
            v = [sizing(level, t, m, k) for m in maxbs]
            assert all(a <= b for a, b in zip(v, v[1:])), ("max_chunk_bytes", t, k)
        for maxb in maxbs:
            v = [sizing(level, t, maxb, k) for k in ks]
            assert all(a <= b for a, b in zip(v, v[1:])), ("nchunks", t, maxb)


@pytest.mark.parametrize("level,top", GOOD)
def test_sizing_never_passes_the_uniform_slots(level, top):
    """whatever the promise: the uniform-slot answer for the same nchunks / max_chunk_bytes and the four arrays"""
    lib = L.lib()
    for maxb in [m for m in FIXED + [63, 64, 32768, 1 << 20] if m <= top]:
        for k in (0, 1, 2, 17, 256, 1000, 4096):
            uniform = lib.lzh_zstd_ragged_compress_temp_bytes(level, maxb, k)
            for total in (0, 1, maxb, k * maxb // 3, k * maxb, 2 * k * maxb + 5, 1 << 40):
                assert sizing(level, total, maxb, k) <= uniform + arrays_bytes(k), (maxb, k, total)


def test_skewed_batch_sizes_to_a_fraction_of_the_uniform_slots():
    """4096 chunks, one of 16 MiB and 4095 of 4 KiB: about 32 MiB of input.  (The figures in the header:
    867,689,472 bytes against 74,381,787,648.)"""
    k, total = 4096, MAX + 4095 * 4096
    compact = sizing(1, total, MAX, k)
    uniform = L.lib().lzh_zstd_ragged_compress_temp_bytes(1, MAX, k)
    print(f"skewed batch: compact {compact}, uniform slots {uniform}")
    assert 0 < compact * 10 < uniform, (compact, uniform)
    # and it is what the text says it is: 24 + 1 + 1/256 bytes per input byte, 7168 + 335 per chunk, the arrays
    assert compact <= 25 * total + total // 256 + k * (7168 + 335) + arrays_bytes(k) + 4 * 256


# ---- the host mirror against the regions --------------------------------------------------------------------------
# The per-frame scratch of the two zstd kernels, restated from csrc/zstdc.h (params_for: the clevels.h rows
# for sizes up to 16 KiB / 128 KiB / 256 KiB / above, levels <= 0 | 1 | 2 as (windowLog, hashLog); layout_for).
ROWS = {3: [(14, 13), (14, 15), (14, 15)], 2: [(17, 12), (17, 13), (17, 15)], 1: [(18, 13), (18, 14), (18, 16)],
        0: [(19, 13), (19, 14), (20, 16)]}


def scratch_need(level, n):
    n = max(n, 1)                                    # (an empty chunk: laid out as a 1-byte chunk)
    tid = (n <= 262144) + (n <= 131072) + (n <= 16384)
    wlog, hlog = ROWS[tid][max(level, 0)]
    srclog = 6 if n < 64 else (n - 1).bit_length()
    wlog = min(wlog, srclog)
    hlog = min(hlog, wlog + 1)
    b = min(1 << max(wlog, 10), 131072, n)
    need = 1024 + a256((b // 4 + 16) * 8) + a256(b + 64) + a256(4 * b + 4096) + a256(b + 256) + (4 << hlog)
    return a256(need)


def test_restated_layout_against_the_uniform_stride():
    """the restatement is the layout the library sizes a uniform call's frames with, where that is a single size's
    (levels whose worst-of-four-levels stride comes from this level: checked through <=)"""
    lib = L.lib()
    for n in [s for s in FIXED if s]:
        per_level = [scratch_need(lv, n) for lv in (1, -1)] + ([scratch_need(2, n)] if n <= 131072 else [])
        uniform = lib.lzh_zstd_ragged_compress_temp_bytes(1, n, 1) - lib.lzh_stage_stride(ZSTD, n) - 512
        assert max(per_level) <= uniform, n
    assert scratch_need(1, 16384) > scratch_need(1, 16385)      # hashLog 15 | 13: the slot is not monotone


def mirror(level, sizes, maxb, total):
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    k = len(sizes)
    so, co, pr = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.uint8)
    rc = L.lib().lzh_debug_zstd_ragged_compact_slots(level, sizes.ctypes.data, k, maxb, total, so.ctypes.data,
                                                     co.ctypes.data, pr.ctypes.data)
    assert rc == OK
    return so.astype(np.int64), co.astype(np.int64), pr.astype(bool)


def regions(level, total, maxb, k):
    """(staging offset, staging bytes, scratch offset, scratch bytes) inside the temp buffer, checked against the
    sizing answer: inside it, disjoint, 256-aligned, the four arrays after them."""
    out = np.zeros(4, np.uint64)
    assert L.lib().lzh_debug_zstd_ragged_compact_regions(level, total, maxb, k, out.ctypes.data) == OK
    s0, sb, c0, cb = (int(v) for v in out)
    ans = sizing(level, total, maxb, k)
    assert s0 % 256 == 0 and c0 % 256 == 0
    assert s0 + sb <= c0 and c0 + cb + arrays_bytes(k) <= ans, (s0, sb, c0, cb, ans)
    return s0, sb, c0, cb


def needs(level, sizes, maxb):
    lib = L.lib()
    st = np.array([lib.lzh_stage_stride(ZSTD, int(n)) if n <= maxb else 0 for n in sizes], np.int64)
    sc = np.array([scratch_need(level, int(n)) if n <= maxb else 0 for n in sizes], np.int64)
    return st, sc


def size_lists(level, top):
    """(sizes, max_chunk_bytes): the fixed list, then seeded random ones -- edge sizes, small chunks with a few
    large ones, all at the largest size, sizes just past the size classes"""
    fixed = [s for s in FIXED if s <= top]
    yield np.array(fixed, np.int64), max(fixed)
    rng = np.random.default_rng(1000 + level)
    edge = [s for s in FIXED if s <= top] + [63, 64, 65, 2048, 32768, 32769]
    for it in range(120):
        maxb = int(rng.choice([m for m in (1, 4096, 16384, 16385, 65536, 131072, 300000, 1 << 20, MAX) if m <= top]))
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
            s = np.minimum(maxb, 2 ** rng.integers(0, 25, k) + rng.integers(0, 3, k))
        yield np.asarray(s, np.int64), maxb


@pytest.mark.parametrize("level,top", GOOD)
def test_a_kept_promise_places_every_slot_inside_its_region(level, top):
    for sizes, maxb in size_lists(level, top):
        k, total = len(sizes), int(sizes.sum())          # the promise spent to the last byte
        for pad in (0, 5):                               # (and buffers sized for more chunks than the batch has)
            szs = np.concatenate([sizes, np.zeros(pad, np.int64)])
            so, co, pr = mirror(level, szs, maxb, total)
            assert pr.all(), (szs, total)
            st, sc = needs(level, szs, maxb)
            _, sb, _, cb = regions(level, total, maxb, len(szs))
            assert (so % 256 == 0).all() and (co % 256 == 0).all() and so[0] == 0 and co[0] == 0
            # in index order, disjoint: the next slot starts at or after this one's end -- for the scratch slot at or
            # after what the kernels need for it, so every slot is at least that
            assert (so[1:] >= so[:-1] + st[:-1]).all() and (co[1:] >= co[:-1] + sc[:-1]).all(), "slots overlap"
            assert int((so + st).max()) <= sb and int((co + sc).max()) <= cb, (szs, total)


@pytest.mark.parametrize("level,top", GOOD)
def test_scratch_slots_are_exactly_the_restated_layout(level, top):
    """(stronger than `at least`: the library spends nothing more than the layout either)"""
    sizes = np.array([s for s in FIXED if s <= top] + [0], np.int64)
    so, co, pr = mirror(level, sizes, int(sizes.max()), int(sizes.sum()))
    st, sc = needs(level, sizes, int(sizes.max()))
    assert pr.all()
    assert (np.diff(so) == st[:-1]).all() and (np.diff(co) == sc[:-1]).all()
    assert scratch_need(level, 0) <= 8192               # an empty chunk does not cost a 128 KiB block's areas


@pytest.mark.parametrize("level,top", GOOD)
def test_a_broken_promise_drops_chunks_and_moves_none(level, top):
    dropped = 0
    for sizes, maxb in size_lists(level, top):
        total = int(sizes.sum())
        if total < 2:
            continue
        so0, co0, pr0 = mirror(level, sizes, maxb, total)
        assert pr0.all()
        so, co, pr = mirror(level, sizes, maxb, total // 2)
        st, sc = needs(level, sizes, maxb)
        _, sb, _, cb = regions(level, total // 2, maxb, len(sizes))
        assert (pr == ((so + st <= sb) & (co + sc <= cb))).all(), (sizes, total)
        assert (so == so0).all() and (co == co0).all()   # the chunks that stay processed keep their offsets
        dropped += int((~pr).sum())
    assert dropped > 0
    # a chunk over max_chunk_bytes takes no slot bytes and is not processed; its neighbours are
    so, co, pr = mirror(level, np.array([100, 4097, 200], np.int64), 4096, 300)
    assert pr.tolist() == [True, False, True] and so[1] == so[2] and co[1] == co[2]


# ---- the debug calls refuse what the async call refuses (its own checks: tests/test_ragged_calls_abi.py) -------------
@pytest.mark.parametrize("level,maxb", [(0, 65536), (3, 65536), (2, 131073), (19, 4096), (1, MAX + 1), (-1, MAX + 1)])
def test_unsupported_level_or_size_comes_first(level, maxb):
    lib = L.lib()
    one = np.zeros(1, np.uint64)
    assert lib.lzh_debug_zstd_ragged_compact_slots(level, one.ctypes.data, 1, maxb, 0, one.ctypes.data, one.ctypes.data,
                                                   one.ctypes.data) == EARG
    assert lib.lzh_debug_zstd_ragged_compact_regions(level, 0, maxb, 1, one.ctypes.data) == EARG
    for lv, m in [(1, 65536), (-5, 300000), (2, 131072), (-1, 0)]:     # (a null output, at supported arguments)
        assert lib.lzh_debug_zstd_ragged_compact_regions(lv, 2 * m + 17, m, 4, None) == EARG


def test_python_value_errors():
    """RaggedCodec's checks come before any torch call: no device needed."""
    with pytest.raises(ValueError, match="zstd option"):
        L.RaggedCodec("lz4", 65536, 4, compact_scratch=True)
    with pytest.raises(ValueError, match="zstd option"):
        L.RaggedCodec("snappy", 65536, 4, compact=True, compact_scratch=True)
    with pytest.raises(ValueError, match="compact_scratch"):
        L.RaggedCodec("zstd", 65536, 4, level=1, compact=True)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd", 131073, 4, level=2, compact_scratch=True)
