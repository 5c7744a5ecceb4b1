"""bench.py's command line: --dump-outputs writes the timed path's last outputs as comparable .npy files, and a plain
run (no --full) reports the headline figure without the checks and baselines that --full adds."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("packed_total", "compr_sizes", "status", "packed_chunk_sums", "out_chunk_sums", "packed_sample", "out_sample")
FULL_ONLY = ("roofline", "roofline_decompress", "cpu_baseline", "cpu_baseline_all_cores", "e2e", "bit_exact",
             "roundtrip_ok", "host_cpu")


def test_dump_outputs_arrays(tmp_path):
    """CPU: the dump of a codec state built with the oracle (ragged last chunk): every array's type and content,
    the same files from a second call, and a size that stays under 64 MB whatever the input size."""
    import bench
    import lzbench_amd as L
    chunk, n = 65536, 3 * 65536 + 1234
    data = L.datagen("text", n, seed=5)
    packed, cs = O.compress_chunks(data, "lz4", chunk)
    k = len(cs)
    offs = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
    pad = np.zeros(64, np.uint8)
    codec = SimpleNamespace(k=k, offsets=torch.from_numpy(offs), packed=torch.from_numpy(np.concatenate([packed, pad])),
                            out=torch.from_numpy(np.concatenate([data, pad])),
                            csizes=torch.from_numpy(cs.astype(np.int32)), status=torch.zeros(k, dtype=torch.int32))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), codec, len(packed), n, chunk, 0, 1)
    bench.dump_outputs(str(b), codec, len(packed), n, chunk, 0, 1)
    assert sorted(os.listdir(a)) == sorted(f"{x}.npy" for x in NAMES)
    got = {x: np.load(a / f"{x}.npy") for x in NAMES}
    for x in NAMES:
        assert got[x].dtype in (np.float32, np.float64), x
        assert np.array_equal(got[x], np.load(b / f"{x}.npy")), x
    assert got["packed_total"].tolist() == [len(packed)]
    assert np.array_equal(got["compr_sizes"], cs.astype(np.float64))
    assert np.array_equal(got["status"], np.zeros(k))
    assert got["packed_chunk_sums"].tolist() == [float(packed[offs[i]:offs[i + 1]].sum(dtype=np.uint64)) for i in range(k)]
    assert got["out_chunk_sums"].tolist() == [float(data[i * chunk:(i + 1) * chunk].sum(dtype=np.uint64)) for i in range(k)]
    assert len(got["packed_sample"]) == len(got["out_sample"]) == bench.DUMP_SAMPLE
    assert set(np.unique(got["out_sample"])) <= set(np.unique(data).astype(np.float32))
    # the samples do not grow with the input; the per-chunk arrays do: 4 x 8 bytes per chunk (1 GiB at -b64: 0.5 MB)
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) < 40e6


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only_and_dumps(tmp_path):
    """one small plain run: --steps sets the timed steps, ms_per_step and value agree, nothing of --full is in the
    line, and the dumped decode matches the corpus the arguments name"""
    import lzbench_amd as L
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--size-mib", "16", "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "MB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx((16 << 20) / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d]
    n, chunk = 16 << 20, 65536
    data = L.datagen("text", n, seed=12345)
    packed, cs = O.compress_chunks(data, "lz4", chunk)
    got = {x: np.load(tmp_path / "d" / f"{x}.npy") for x in NAMES}
    assert got["packed_total"].tolist() == [len(packed)]
    assert np.array_equal(got["compr_sizes"], cs.astype(np.float64))
    assert (got["status"] >= 0).all()
    assert np.array_equal(got["out_chunk_sums"], data.reshape(-1, chunk).sum(axis=1, dtype=np.uint64).astype(np.float64))
    offs = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
    assert np.array_equal(got["packed_chunk_sums"], np.add.reduceat(packed, offs[:-1], dtype=np.uint64).astype(np.float64))
