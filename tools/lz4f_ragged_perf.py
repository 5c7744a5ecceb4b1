"""tools/lz4f_ragged_perf.py [OUT.json] -- the ragged LZ4 frame calls (include/lzbench_hip.h 3i) next to the uniform
LZ4 frame calls on the same device-resident bytes in one process: 4,096 chunks of 256 KiB of datagen text at level 4
(64 KiB blocks, four a frame).  Per direction:
  ragged_compress / ragged_decompress      lzh_lz4f_compress_ragged_async / lzh_lz4f_decompress_ragged_async
  uniform_compress / uniform_decompress    lzh_compress_async / lzh_decompress_async with LZH_CODEC_LZ4F
  uniform_compress_again / uniform_decompress_again   the uniform calls a second time in every round: the distance
                                           between the two medians is the uniform call's own run-to-run spread
The ragged calls run the uniform calls' parse, emit and block-decode kernels over the same blocks plus one small table
kernel, so the expectation is ragged = uniform within 5 % beyond that spread; `verdict` records both figures.  The
packed bytes of the two must be equal, the decoders' outputs are compared with the input.
Then one skewed batch, one 16 MiB chunk among 4,095 of 4 KiB with max_chunk_bytes = 16 MiB: its compress temp (uniform
slots: every frame pays for the largest chunk) and, where that temp fits in half of the free device memory, its time.
HIP events around each call, 3 warm-up and 20 timed rounds, all variants alternating inside every round; medians with
their range."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lzbench_amd as L  # noqa: E402
from perf_rounds import alternate, stats  # noqa: E402

WARM, REP = 3, 20
LEVEL = 4


def measure(k, chunk):
    n = k * chunk
    host = L.datagen("text", n, seed=4242)
    d_in = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(torch.from_numpy(host))
    offs, sizes = np.arange(k, dtype=np.int64) * chunk, np.full(k, chunk, np.int64)
    rc = L.RaggedCodec("lz4frame", chunk, k, level=LEVEL)
    dc = L.DeviceCodec("lz4frame", n, chunk, level=LEVEL)
    out = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    src, dst = rc._arrays(d_in, offs, sizes, 16)[0], rc._arrays(out, offs, sizes, 0)[0]
    runs = {"ragged_compress": lambda: rc.compress_arrays(src, k), "uniform_compress": lambda: dc.compress(d_in),
            "uniform_compress_again": lambda: dc.compress(d_in),
            "ragged_decompress": lambda: rc.decompress_arrays(dst, k), "uniform_decompress": dc.decompress,
            "uniform_decompress_again": dc.decompress}
    t = alternate(runs, WARM, REP)
    torch.cuda.synchronize()
    res = {"chunks": k, "chunk_bytes": chunk, "input_bytes": n, "level": LEVEL, "warmup": WARM, "repeats": REP}
    for key in runs:
        res[key] = stats(t[key], n)
    total = rc.packed_total()
    assert total == dc.packed_total() and torch.equal(rc.packed[:total], dc.packed[:total]), "packed bytes differ"
    assert torch.equal(out[:n], d_in[:n]) and torch.equal(dc.out[:n], d_in[:n])
    assert bool((rc.status[:k] == chunk).all())
    res["packed_bytes"] = total
    res["ragged_compress_temp_bytes"], res["uniform_compress_temp_bytes"] = rc.ctemp.numel(), dc.ctemp.numel()
    res["ragged_decompress_temp_bytes"], res["uniform_decompress_temp_bytes"] = rc.dtemp.numel(), dc.dtemp.numel()
    for d in ("compress", "decompress"):
        u, u2, r = (res[f"{v}_{d}"]["median_ms"] for v in ("uniform", "uniform", "ragged"))
        u2 = res[f"uniform_{d}_again"]["median_ms"]
        spread = abs(u - u2) / min(u, u2)
        gap = r / min(u, u2) - 1
        res[f"{d}_verdict"] = {"ragged_over_uniform": r / min(u, u2), "uniform_spread": spread, "gap": gap,
                               "within_5_percent_beyond_spread": bool(gap <= 0.05 + spread)}
    return res


def skewed(k, big, small):
    lib = L.lib()
    res = {"chunks": k, "largest_chunk_bytes": big, "other_chunk_bytes": small, "input_bytes": big + (k - 1) * small,
           "level": LEVEL, "compress_temp_bytes": lib.lzh_lz4f_ragged_compress_temp_bytes(LEVEL, big, k),
           "decompress_temp_bytes": lib.lzh_lz4f_ragged_decompress_temp_bytes(big, k)}
    free, _ = torch.cuda.mem_get_info()
    res["free_device_bytes"] = free
    if res["compress_temp_bytes"] > free // 2:
        res["timed"] = False
        res["why_not"] = "the compress temp exceeds half of the free device memory"
        return res
    sizes = np.full(k, small, np.int64)
    sizes[k // 2] = big
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    n = int(sizes.sum())
    host = L.datagen("text", n, seed=77)
    d_in = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(torch.from_numpy(host))
    out = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    rc = L.RaggedCodec("lz4frame", big, k, level=LEVEL, max_total_bytes=n)
    src, dst = rc._arrays(d_in, offs, sizes, 16)[0], rc._arrays(out, offs, sizes, 0)[0]
    t = alternate({"compress": lambda: rc.compress_arrays(src, k), "decompress": lambda: rc.decompress_arrays(dst, k)},
                  WARM, REP)
    torch.cuda.synchronize()
    assert torch.equal(out[:n], d_in[:n])
    res.update(timed=True, compress=stats(t["compress"], n), decompress=stats(t["decompress"], n),
               packed_bytes=rc.packed_total())
    return res


def main():
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0)}
    out["text-4096x256KiB"] = measure(4096, 262144)
    print("text-4096x256KiB", json.dumps(out["text-4096x256KiB"]), flush=True)
    torch.cuda.empty_cache()
    out["skewed-1x16MiB+4095x4KiB"] = skewed(4096, 16 << 20, 4096)
    print("skewed", json.dumps(out["skewed-1x16MiB+4095x4KiB"]), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
