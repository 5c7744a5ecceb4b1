"""tools/zstd_ragged_split_compact_perf.py [OUTDIR] -- the measurement of DESIGN.md section 5 for the ragged zstd
split decoder in the compact temp layout (include/lzbench_hip.h 3g), zstd level 1, HIP events, 3 warm-up and 20 timed
calls each (median, min, max):
  a. 4,096 x 128 KiB mixed: the compact call between two series of 3c's uniform-slot split call, same process;
  b. one 16 MiB chunk + 4,095 x 4 KiB: the compact call and the one-wave decoder (3c's split temp would be 142 GB);
  c. 512 MiB in sizes spread from 16 KiB to 1 MiB (seed 7): the one-wave decoder, 3c's split call, the compact call.
Writes OUTDIR/perf.json (default: profiles/zstd_ragged_split_compact/ in the repository root)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lzbench_amd as L  # noqa: E402

LEVEL, WARM, RUNS = 1, 3, 20
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "zstd_ragged_split_compact")
os.makedirs(OUT, exist_ok=True)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()))


def batch(sizes, seed):
    """the chunks back to back (16 bytes apart) in one device buffer of mixed data"""
    sizes = np.asarray(sizes, np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes + 16)[:-1]]).astype(np.int64)
    n = int(offs[-1] + sizes[-1]) + 256
    host = L.datagen("mixed", n, seed=seed)
    return torch.from_numpy(host).cuda(), offs, sizes, n


def case(name, sizes, seed, decoders):
    d_in, offs, sizes, n = batch(sizes, seed)
    k, maxb, total = len(sizes), int(sizes.max()), int(sizes.sum())
    base = L.RaggedCodec("zstd", maxb, k, LEVEL, max_total_bytes=total, compact_scratch=True)
    base.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_dst, _ = base._arrays(out, offs, sizes, 0)
    res = dict(chunks=k, max_chunk_bytes=maxb, total_bytes=total, packed_bytes=base.packed_total())
    flags = {"onewave": {}, "split_uniform": dict(split_decode=True),
             "split_compact": dict(split_decode=True, compact_decode=True)}
    lib = L.lib()
    for tag, dec in decoders:
        if dec == "split_uniform" and lib.lzh_zstd_ragged_decompress_split_temp_bytes(maxb, k) > (64 << 30):
            continue
        # (decode only: compact_scratch keeps the compress temp these codecs never use at the batch's size, not
        # nchunks x the slot of the largest chunk)
        rc = L.RaggedCodec("zstd", maxb, k, LEVEL, max_total_bytes=total, compact_scratch=True, **flags[dec])
        res[tag + "_temp_bytes"] = int(rc.dtemp.numel())
        out.zero_()
        fn = lambda: rc.decompress_arrays(d_dst, k, packed=base.packed, csizes=base.csizes, offsets=base.offsets)  # noqa: E731
        res[tag] = timed(fn)
        ok = bool((rc.status[:k].cpu().numpy() == sizes).all())
        for i in (0, k // 2, k - 1, int(sizes.argmax())):
            ok = ok and torch.equal(out[offs[i]: offs[i] + sizes[i]], d_in[offs[i]: offs[i] + sizes[i]])
        res[tag + "_ok"] = ok
        if dec == "split_compact":   # (region 3 of the layout: 2 = finished by the split kernels, 3 = by the one-wave kernel)
            v = np.zeros(23, np.uint64)
            assert lib.lzh_debug_zstd_ragged_split_compact_layout(total, maxb, k, v.ctypes.data) == 0
            st = rc.dtemp[int(v[6]): int(v[6]) + 4 * k].cpu().numpy().view(np.int32)
            res[tag + "_frames_by_state"] = {str(int(a)): int(b) for a, b in zip(*np.unique(st, return_counts=True))}
        del rc, fn
        torch.cuda.empty_cache()
    print(name, json.dumps(res), flush=True)
    return res


def main():
    torch.cuda.set_device(0)
    rng = np.random.default_rng(7)
    spread = []
    while sum(spread) < (512 << 20):
        spread.append(int(np.exp(rng.uniform(np.log(16384), np.log(1 << 20)))))
    res = dict(level=LEVEL, warmup=WARM, runs=RUNS, corpus="mixed")
    a = case("a", [131072] * 4096, 1, [("split_uniform_a", "split_uniform"), ("split_compact", "split_compact"),
                                       ("split_uniform_b", "split_uniform")])
    # "equal": the compact call's median within the min-max spread of the uniform-slot call's own timings
    lo = min(a["split_uniform_a"]["min_ms"], a["split_uniform_b"]["min_ms"])
    hi = max(a["split_uniform_a"]["max_ms"], a["split_uniform_b"]["max_ms"])
    a["compact_median_within_uniform_spread"] = bool(lo <= a["split_compact"]["median_ms"] <= hi)
    res["a_4096x128KiB"] = a
    res["b_16MiB_and_4095x4KiB"] = case("b", [4096] * 5 + [16 << 20] + [4096] * 4090, 2,
                                        [("onewave", "onewave"), ("split_compact", "split_compact")])
    res["c_512MiB_16KiB_to_1MiB"] = case("c", spread, 3, [("onewave", "onewave"), ("split_uniform", "split_uniform"),
                                                          ("split_compact", "split_compact")])
    with open(os.path.join(OUT, "perf.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
