"""GPU zstd compression (the hip_zstd / hip_zstd_fast rows, lzbench_amd/csrc/zstdc_hip.hip) against
the reference: every digest of tests/golden/zstd_cgolden.json (the reference zstd 1.5.2 build
through lzbench's chunk loop) reproduced byte for byte through the batched C-ABI rows, fresh
inputs equal to the oracle restatement (pinned to the reference by tests/test_zstd_oracle.py),
the per-chunk lzbench rows, and round trips through the GPU decoder.  Run with -m gpu."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
from gpu_batches import sha, torch_cuda

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cgolden():
    with open(os.path.join(GOLD, "zstd_cgolden.json")) as f:
        return json.load(f)["cases"]


def corpus(kind, n, seed):
    if kind == "zeros":
        d = np.zeros(n, np.uint8)
        d[::4099] = 7
        return d
    if kind == "zero":
        return np.zeros(n, np.uint8)
    if kind == "runs":
        rng = np.random.default_rng(seed)
        return np.repeat(rng.integers(0, 4, n // 8 + 16, dtype=np.uint8),
                         rng.integers(1, 300, n // 8 + 16))[:n].copy()
    return L.datagen(kind, n, seed)


def row_name(level):
    return "zstd_fast" if level < 0 else "zstd"


@pytest.mark.parametrize("case", cgolden(), ids=lambda c: f"{c['corpus']}-{c['n']}-b{c['chunk'] >> 10}-l{c['level']}")
def test_batched_row_reproduces_reference_digest(torch_cuda, case):
    data = corpus(case["corpus"], case["n"], case["seed"])
    packed, cs = L.compress_chunks(data, row_name(case["level"]), case["chunk"], level=case["level"])
    assert len(packed) == case["packed_bytes"]
    assert sha(cs.astype("<u8")) == case["csizes_sha256"]
    assert sha(packed) == case["packed_sha256"]
    out = L.decompress_chunks(packed, cs, len(data), "zstd", case["chunk"])
    assert (out == data).all()


@pytest.mark.parametrize("level", [1, -1, -3])
def test_random_slices_equal_oracle(torch_cuda, level):
    rng = np.random.default_rng(level + 7)
    src = np.concatenate([L.datagen("mixed", 1 << 21, seed=3), corpus("runs", 1 << 20, 4),
                          rng.integers(0, 3, 1 << 19, dtype=np.uint8), L.datagen("json", 1 << 20, seed=1)])
    for _ in range(10):
        n = int(rng.integers(1, 900_000))
        off = int(rng.integers(0, len(src) - n))
        chunk = int(rng.choice([65536, 131072, 262144, 524288, 1 << 20]))
        data = src[off:off + n].copy()
        ep, ec = O.compress_chunks(data, "zstd", chunk, level, use_ref=False)
        gp, gc = L.compress_chunks(data, row_name(level), chunk, level=level)
        assert (gc == ec).all() and gp.tobytes() == ep.tobytes(), (n, chunk, level)


def test_device_resident_b128(torch_cuda):
    torch = torch_cuda
    n, chunk = (48 << 20) + 333, 131072
    data = L.datagen("mixed", n, seed=12345)
    d_in = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(torch.from_numpy(data))
    dc = L.DeviceCodec("zstd", n, chunk, level=1)
    dc.compress(d_in)
    dc.decompress()
    torch.cuda.synchronize()
    total = dc.packed_total()
    ep, ec = O.compress_chunks(data, "zstd", chunk, 1, use_ref=False, threads=8)
    assert total == len(ep)
    assert (dc.csizes.cpu().numpy().astype(np.uint64) == ec).all()
    assert (dc.packed[:total].cpu().numpy() == ep).all()
    assert (dc.status.cpu().numpy() >= 0).all() and torch.equal(dc.out[:n], d_in[:n])


def test_per_chunk_rows(torch_cuda):
    lib = L.lib()
    data = L.datagen("text", 131072, seed=9)
    for level in (1, 2, -2):
        wm = lib.lzbench_hip_zstd_init(131072, level & 0xFFFFFFFFFFFFFFFF, 1)
        assert wm
        try:
            out = np.zeros(L.get_compress_bound(131072), np.uint8)
            clen = lib.lzbench_hip_zstd_compress(data.ctypes.data, 131072, out.ctypes.data, len(out),
                                                 level & 0xFFFFFFFFFFFFFFFF, 0, wm)
            ep, ec = O.compress_chunks(data, "zstd", 131072, level, use_ref=False)
            assert clen == len(ep) and out[:clen].tobytes() == ep.tobytes()
            back = np.zeros(131072 + 64, np.uint8)
            assert lib.lzbench_hip_zstd_decompress(out.ctypes.data, clen, back.ctypes.data, 131072, 0, 0, wm) == 131072
            assert (back[:131072] == data).all()
        finally:
            lib.lzbench_hip_deinit(wm)


def test_unsupported_level_rejected(torch_cuda):
    import torch
    dc = L.DeviceCodec("zstd", 1 << 20, 131072, level=3)      # zstd -3 is the dfast strategy
    d_in = torch.zeros((1 << 20) + 256, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        dc.compress(d_in)


def test_huffman_sort_cutoff_chunk(torch_cuda):
    """The GPU Huffman build quick-sorts the same HUF_sort regions as the reference (cutoff 165,
    huf_compress.c:455): chunk 11359 of the 4 GiB config-5 corpus, whose nine symbols of count 164 the
    reference reorders (tests/test_zstd_oracle.py::test_huffman_sort_cutoff_equals_reference)."""
    import test_zstd_oracle as T
    d = T.mixed_chunk_11359()
    packed, cs = L.compress_chunks(d, "zstd", 131072, 1)
    ep, ecs = O.compress_chunks(d, "zstd", 131072, 1)
    assert (cs == ecs).all() and len(packed) == len(ep) and (packed == ep).all()
