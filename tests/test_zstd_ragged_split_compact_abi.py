"""CPU: the compact temp layout of the ragged zstd split decoder (the two debug calls of include/lzbench_hip.h 3c,
lzh_debug_zstd_ragged_split_compact_layout / _slots; host arithmetic, no decode call takes the layout yet): the
properties of the layout's total, its regions, and the placement of areas and job slots."""
import json
import os

import numpy as np

import lzbench_amd as L

OK, EARG = 0, -1
KB, MB = 1 << 10, 1 << 20
MAX = 16 * MB
SPLIT_MIN = 16384
BLOCK = 128 * KB
MAXES = [SPLIT_MIN, 16385, 65536, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1, 300000, MB, MAX]   # (the size-class edges)
COUNTS = [0, 1, 2, 7, 8, 9, 255, 256, 257, 4096]
TOTALS = [0, 1, 4 * KB, SPLIT_MIN, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, MB, MAX, MAX + 4095 * 4 * KB, 1 << 30, 1 << 36]
REGIONS = ["offsets", "areas", "dummy", "states", "fields", "njobs", "jobs", "area_sz", "job_cnt", "area_off", "job_off"]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sizing_zstd_split_compact.json")


def compact_bytes(total, maxb, k):
    """the layout's total (0 where the layout call refuses the size)"""
    rc, v = temp_layout(total, maxb, k)
    return v[22] if rc == OK else 0


def split_bytes(maxb, k):
    return L.lib().lzh_zstd_ragged_decompress_split_temp_bytes(maxb, k)


def arrays_bytes(k):
    """the four per-chunk arrays, each rounded up to 256: two u32 of k, two u64 of k + 1"""
    al = lambda v: (v + 255) // 256 * 256
    return 2 * al(4 * k) + 2 * al(8 * (k + 1))


def temp_layout(total, maxb, k):
    out = np.zeros(23, np.uint64)
    rc = L.lib().lzh_debug_zstd_ragged_split_compact_layout(total, maxb, k, out.ctypes.data)
    return rc, [int(v) for v in out]


def uniform_layout(maxb, k):
    out = np.zeros(16, np.uint64)
    assert L.lib().lzh_debug_zstd_ragged_split_layout(maxb, k, out.ctypes.data) == OK
    return [int(v) for v in out]


def bmax(n):
    """block slots (= Huffman job slots) of a frame of n bytes"""
    return (n + BLOCK - 1) // BLOCK + 1


def stride(n):
    """the area of a frame of n bytes (the issue's figures: 26,368 bytes at 4 KiB, 34,685,184 at 16 MiB)"""
    return (bmax(n) * 8760 + (n // 4 + 64) * 8 + 255) // 256 * 256


def job_bytes():
    """a Huffman job's bytes, from the uniform-slot layout: one frame of 16 KiB has bmax(16384) = 2 job slots"""
    return uniform_layout(SPLIT_MIN, 1)[13] // bmax(SPLIT_MIN)


def _self_check():
    """(of this file's helpers, not of the change: stride() restates the uniform-slot layout's frame area)"""
    for maxb in MAXES:
        assert uniform_layout(maxb, 3)[14] == stride(maxb), maxb
    assert stride(MAX) == 34_685_184 and stride(4 * KB) == 26_368



def mirror(sizes, maxb, total):
    k = len(sizes)
    s = np.array(sizes, np.uint64)
    off = np.zeros(k, np.uint64)
    job = np.zeros(k, np.uint64)
    ins = np.zeros(k, np.uint8)
    rc = L.lib().lzh_debug_zstd_ragged_split_compact_slots(s.ctypes.data, k, maxb, total, off.ctypes.data, job.ctypes.data,
                                                          ins.ctypes.data)
    assert rc == OK
    return [int(v) for v in off], [int(v) for v in job], [int(v) for v in ins]


def test_zero_exactly_where_the_uniform_slot_answer_is():
    for maxb in [0, 1, SPLIT_MIN - 1, SPLIT_MIN, 70000, MAX, MAX + 1, 1 << 30]:
        for k in (0, 1, 9, 4096):
            for total in (0, 1, MB, 1 << 36):
                assert (compact_bytes(total, maxb, k) == 0) == (split_bytes(maxb, k) == 0), (total, maxb, k)


def test_sizing_is_monotone_in_each_argument():
    for maxb in MAXES:
        for k in COUNTS:
            prev = 0
            for total in TOTALS:
                v = compact_bytes(total, maxb, k)
                assert v >= prev and v > 0, (total, maxb, k)
                prev = v
    for total in TOTALS:
        for k in COUNTS:
            prev = 0
            for maxb in MAXES:
                v = compact_bytes(total, maxb, k)
                assert v >= prev, (total, maxb, k)
                prev = v
        for maxb in MAXES:
            prev = 0
            for k in COUNTS:
                v = compact_bytes(total, maxb, k)
                assert v >= prev, (total, maxb, k)
                prev = v


def test_never_above_the_uniform_slot_answer_plus_the_four_arrays():
    for maxb in MAXES:
        for k in COUNTS:
            for total in TOTALS:
                assert compact_bytes(total, maxb, k) <= split_bytes(maxb, k) + arrays_bytes(k), (total, maxb, k)
            # a total that no batch of k chunks passes: exactly the uniform layout and the arrays
            assert compact_bytes(k * maxb, maxb, k) == split_bytes(maxb, k) + arrays_bytes(k), (maxb, k)


def test_skewed_batch():
    _self_check()
    k = 4096
    total = MAX + (k - 1) * 4 * KB
    v, u = compact_bytes(total, MAX, k), split_bytes(MAX, k)
    print("skewed batch:", v, "uniform slots:", u)
    assert 0 < v < u // 100
    # the areas those frames need fit (the issue's ~143 MB) and the answer is of that order
    need = stride(MAX) + (k - 1) * stride(4 * KB)
    assert need <= v <= need + 4 * MB


def test_regions_are_disjoint_aligned_and_in_order():
    for total, maxb, k in [(0, SPLIT_MIN, 0), (MAX + 4095 * 4 * KB, MAX, 4096), (9 * 70000, 70000, 9), (MB, BLOCK, 1000),
                           (1 << 36, 300000, 1000), (5, MAX, 1)]:
        rc, v = temp_layout(total, maxb, k)
        assert rc == OK
        end = 0
        for i, name in enumerate(REGIONS):
            off, size = v[2 * i], v[2 * i + 1]
            assert off % 256 == 0 and off >= end, (total, maxb, k, name)    # (in the stated order, no overlap)
            end = off + size
        assert end <= v[22] < end + 256                                     # the last region ends the temp
        assert v[22] == compact_bytes(total, maxb, k)
        by = {n: (v[2 * i], v[2 * i + 1]) for i, n in enumerate(REGIONS)}
        assert by["offsets"] == (0, 8 * (k + 1))                           # where the other ragged calls scan them to
        assert by["states"][1] == 4 * k and by["njobs"][1] == 4
        assert by["area_sz"][1] == by["job_cnt"][1] == 4 * k
        assert by["area_off"][1] == by["job_off"][1] == 8 * (k + 1)
        assert by["areas"][1] % 256 == 0 and by["areas"][1] <= k * stride(maxb)
        assert by["jobs"][1] == job_bytes() * min(total // BLOCK + 2 * k, k * bmax(maxb))
    out = np.zeros(23, np.uint64)
    lib = L.lib()
    assert lib.lzh_debug_zstd_ragged_split_compact_layout(MB, SPLIT_MIN - 1, 4, out.ctypes.data) == EARG
    assert lib.lzh_debug_zstd_ragged_split_compact_layout(MB, MAX + 1, 4, out.ctypes.data) == EARG
    assert lib.lzh_debug_zstd_ragged_split_compact_layout(MB, 65536, 4, None) == EARG


def test_host_placement_mirror():
    _self_check()
    rng = np.random.default_rng(20261020)
    jb = job_bytes()
    broken_by_jobs = 0
    for b in range(200):
        maxb = int(rng.choice([SPLIT_MIN, BLOCK, BLOCK + 1, MB, 2 * MB]))
        menu = [s for s in (0, 1, 4 * KB, 16 * KB, BLOCK, BLOCK + 1, MB, maxb) if s <= maxb]
        k = int(rng.integers(1, 40))
        sizes = [int(rng.choice(menu)) for _ in range(k)]
        total = sum(sizes)
        want = [int(w) for w in np.concatenate([[0], np.cumsum([stride(s) for s in sizes])])]
        wantj = [int(w) for w in np.concatenate([[0], np.cumsum([bmax(s) for s in sizes])])]
        assert all(w % 256 == 0 for w in want)
        # the promise kept: every chunk in the split kernels; areas and job slots the exclusive scans of the frames'
        # own strides and block slots (so they are disjoint), all inside their regions
        off, job, ins = mirror(sizes, maxb, total)
        v = temp_layout(total, maxb, k)[1]
        assert ins == [1] * k, (b, sizes, maxb)
        assert off == want[:-1] and job == wantj[:-1]
        assert want[-1] <= v[3] and wantj[-1] * jb <= v[13]
        # the promise broken: the same scans, and in_split exactly where both ends are inside the smaller regions
        half = total // 2
        off2, job2, ins2 = mirror(sizes, maxb, half)
        v2 = temp_layout(half, maxb, k)[1]
        assert off2 == off and job2 == job
        for i in range(k):
            area_in = off2[i] + stride(sizes[i]) <= v2[3]
            jobs_in = (job2[i] + bmax(sizes[i])) * jb <= v2[13]
            assert bool(ins2[i]) == (area_in and jobs_in), (b, i, area_in, jobs_in)
            broken_by_jobs += area_in and not jobs_in
        # a chunk over max_chunk_bytes takes 0 bytes and 0 slots and is not in the split kernels
        j = int(rng.integers(0, k))
        over = list(sizes)
        over[j] = maxb + 1
        off3, job3, ins3 = mirror(over, maxb, total)
        assert ins3[j] == 0
        assert off3[: j + 1] == off[: j + 1] and job3[: j + 1] == job[: j + 1]
        assert off3[j + 1:] == [o - stride(sizes[j]) for o in off[j + 1:]]
        assert job3[j + 1:] == [o - bmax(sizes[j]) for o in job[j + 1:]]
        assert all(ins3[i] for i in range(k) if i != j)
    # (No batch here is kept out by the job list alone: a broken promise takes 2 bytes of area region away for
    # every byte, and one job slot for every 128 KiB, so the area region runs out first.  The job condition is
    # still part of in_split, and the comparison above holds it to the region either way.)
    print("frames kept out by the job list alone:", broken_by_jobs)


def test_sizing_goldens():
    with open(GOLD) as f:
        gold = json.load(f)
    assert len(gold["answers"]) >= 12
    for row in gold["answers"]:
        got = compact_bytes(row["total"], row["max"], row["nchunks"])
        assert got == row["bytes"], (row, got)

