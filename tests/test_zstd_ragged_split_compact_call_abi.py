"""CPU: the sizing function of the ragged zstd split decoder's compact call (include/lzbench_hip.h 3g; the call's
argument checks: tests/test_ragged_calls_abi.py)."""
import numpy as np

import lzbench_amd as L

MIB = 1 << 20
LZH_OK, LZH_EARG = 0, -1          # (include/lzbench_hip.h)


def sizing(total, maxb, k):
    return L.lib().lzh_zstd_ragged_decompress_split_compact_temp_bytes(total, maxb, k)


def layout_total(total, maxb, k):
    v = np.zeros(23, np.uint64)
    rc = L.lib().lzh_debug_zstd_ragged_split_compact_layout(total, maxb, k, v.ctypes.data)
    return rc, int(v[22])


def test_sizing_answers():
    # the header's two worked examples
    assert sizing(16 * MIB + 4095 * 4096, 16 * MIB, 4096) == 145_583_104
    assert sizing(4096 * 131072, 131072, 4096) == 1_149_519_360
    totals = [0, 1, 4096, 131072, 131073, 5 * MIB, 33_550_336, 1 << 30]
    maxbs = [16384, 65536, 131072, 131073, 300000, 2 * MIB, 16 * MIB]
    ks = [1, 2, 7, 64, 4096]
    for t in totals:
        for m in maxbs:
            for k in ks:
                rc, want = layout_total(t, m, k)
                assert rc == LZH_OK and sizing(t, m, k) == want > 0, (t, m, k)
    for m in (16383, 16 * MIB + 1):
        assert layout_total(1 << 20, m, 8)[0] == LZH_EARG
        assert sizing(1 << 20, m, 8) == 0
    # non-decreasing along each axis
    for m in maxbs:
        for k in ks:
            a = [sizing(t, m, k) for t in totals]
            assert a == sorted(a), ("total", m, k)
    for t in totals:
        for k in ks:
            a = [sizing(t, m, k) for m in maxbs]
            assert a == sorted(a), ("max", t, k)
        for m in maxbs:
            a = [sizing(t, m, k) for k in ks]
            assert a == sorted(a), ("nchunks", t, m)


def test_skewed_batch_sizing_is_arithmetic():
    """64 chunks, one of 2 MiB among 4 KiB ones (the batch of the GPU tests): by the header's formulas the compact
    answer is about 6 MB and the uniform-slot answer about 278 MB."""
    sizes = [4096] * 64
    sizes[5] = 2 * MIB
    total, maxb, k = sum(sizes), max(sizes), len(sizes)
    uniform = L.lib().lzh_zstd_ragged_decompress_split_temp_bytes(maxb, k)
    compact = sizing(total, maxb, k)
    print("skewed batch: compact", compact, "uniform", uniform)
    assert 0 < compact * 10 < uniform
