"""GPU zstd compression at level 3 (the hip_zstd_dfast row, LZH_CODEC_ZSTD_DFAST, lzbench_amd/csrc/zstdc_dfast_hip.hip)
against the reference: every digest of tests/golden/zstd_dfast_golden.json (the reference zstd 1.5.2 build through
lzbench's chunk loop) reproduced byte for byte through the batched rows and decoded back under both zstd codec names,
fresh slices and a device-resident batch equal to the reference build byte for byte (those two need oracle/_ref),
the per-chunk row, and the level check.  Run with -m gpu."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
from gpu_batches import sha, torch_cuda
import zstd_dfast_cases as Z

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    with open(os.path.join(GOLD, "zstd_dfast_golden.json")) as f:
        return json.load(f)["cases"]


def need_ref():
    if not O.have_ref():
        pytest.skip("reference build (oracle/_ref) not present")


@pytest.mark.parametrize("case", golden(), ids=lambda c: c["name"])
def test_batched_row_reproduces_reference_digest(torch_cuda, case):
    data = Z.corpus(case["corpus"], case["n"], case["seed"])
    assert sha(data) == case["input_sha256"]
    sizes = Z.chunk_list(case["n"], case["chunk"])
    packed, cs = L.compress_chunks(data, "zstd_dfast", case["chunk"], level=3, chunk_sizes=sizes)
    assert len(packed) == case["packed_bytes"]
    assert sha(cs.astype("<u8")) == case["csizes_sha256"]
    assert sha(packed) == case["packed_sha256"]
    for codec in ("zstd_dfast", "zstd") if case["n"] else ():   # (the rows decode nothing for an empty input)
        out = L.decompress_chunks(packed, cs, len(data), codec, case["chunk"], chunk_sizes=sizes)
        assert (out == data).all(), codec


def test_random_slices_equal_reference_build(torch_cuda):
    need_ref()
    rng = np.random.default_rng(33)
    src = np.concatenate([L.datagen("mixed", 1 << 21, seed=3), Z.corpus("runs", 1 << 19, 4),
                          rng.integers(0, 3, 1 << 18, dtype=np.uint8), L.datagen("json", 1 << 20, seed=1)])
    for _ in range(12):
        n = int(rng.integers(1, 900_000))
        off = int(rng.integers(0, len(src) - n))
        chunk = int(rng.choice([16384, 65536, 131072, 262144, 1 << 20]))
        data = src[off:off + n].copy()
        ep, ec = O.compress_chunks(data, "zstd", chunk, 3, use_ref=True)
        gp, gc = L.compress_chunks(data, "zstd_dfast", chunk, level=3)
        assert (gc == ec).all() and gp.tobytes() == ep.tobytes(), (n, off, chunk)


def test_device_resident_b128(torch_cuda):
    need_ref()
    torch = torch_cuda
    n, chunk = (6 << 20) + 333, 131072
    data = L.datagen("mixed", n, seed=12345)
    d_in = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(torch.from_numpy(data))
    dc = L.DeviceCodec("zstd_dfast", n, chunk, level=3)
    assert dc.dtemp.numel() >= L.lib().lzh_decompress_temp_bytes(L.LZH_CODEC_ZSTD, n, chunk)   # the split decoder's temp
    dc.compress(d_in)
    dc.decompress()
    torch.cuda.synchronize()
    total = dc.packed_total()
    ep, ec = O.compress_chunks(data, "zstd", chunk, 3, use_ref=True, threads=8)
    assert total == len(ep)
    assert (dc.csizes.cpu().numpy().astype(np.uint64) == ec).all()
    assert (dc.packed[:total].cpu().numpy() == ep).all()
    assert (dc.status.cpu().numpy() >= 0).all() and torch.equal(dc.out[:n], d_in[:n])


def test_per_chunk_row_and_batched_row(torch_cuda):
    lib = L.lib()
    n = 131072
    data = L.datagen("text", n, seed=9)
    bp, bc = L.compress_chunks(data, "zstd_dfast", n, level=3)           # the batched row, through the init's codec
    assert len(bc) == 1 and int(bc[0]) == len(bp) < n
    wm = lib.lzbench_hip_zstd_dfast_init(n, 3, 1)
    assert wm
    try:
        out = np.zeros(L.get_compress_bound(n), np.uint8)
        clen = lib.lzbench_hip_zstd_dfast_compress(data.ctypes.data, n, out.ctypes.data, len(out), 3, 0, wm)
        assert clen == len(bp) and out[:clen].tobytes() == bp.tobytes()
        if O.have_ref():
            ep, _ = O.compress_chunks(data, "zstd", n, 3, use_ref=True)
            assert out[:clen].tobytes() == ep.tobytes()
        back = np.zeros(n + 64, np.uint8)
        assert lib.lzbench_hip_zstd_decompress(out.ctypes.data, clen, back.ctypes.data, n, 0, 0, wm) == n
        assert (back[:n] == data).all()
        # another level through the row: refused (lzbench stores the chunk raw)
        assert lib.lzbench_hip_zstd_dfast_compress(data.ctypes.data, n, out.ctypes.data, len(out), 1, 0, wm) == 0
    finally:
        lib.lzbench_hip_deinit(wm)


@pytest.mark.parametrize("level", [1, 4])
def test_other_levels_rejected(torch_cuda, level):
    import torch
    dc = L.DeviceCodec("zstd_dfast", 1 << 20, 131072, level=level)
    d_in = torch.zeros((1 << 20) + 256, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        dc.compress(d_in)
