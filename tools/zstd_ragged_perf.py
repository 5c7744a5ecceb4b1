"""tools/zstd_ragged_perf.py [OUTDIR] -- the measurement of profiles/ragged/README.md, last section: 1 GiB mixed
as 8,192 entries of 128 KiB, zstd level 1, through the ragged zstd calls and the uniform ones (HIP events, 2 warm-up
and 12 timed calls each; the uniform call before and after the ragged one, like for like -- one stream, one-wave
decoder -- then with its defaults; then the split-decode series: the ragged call with the split temp between two
series of the uniform split decoder on one stream (lzh_debug_zstd_side(0): the kernels the ragged call shares), the
ragged one-wave call in the same run, and the uniform default).  Writes OUTDIR/zstd_ragged_perf.json (default: bench_out/ in the repository root)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lzbench_amd as L  # noqa: E402

N, CHUNK, LEVEL, RUNS = 1 << 30, 131072, 1, 12
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_out")
os.makedirs(OUT, exist_ok=True)


def timed(fn):
    for _ in range(2):
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
    return dict(median=float(np.median(ts)), min=float(ts.min()), max=float(ts.max()))


def main():
    torch.cuda.set_device(0)
    lib = L.lib()
    host = L.datagen("mixed", N, seed=1)
    d_in = torch.zeros(N + 256, dtype=torch.uint8, device="cuda")
    d_in[:N].copy_(torch.from_numpy(host))
    k = N // CHUNK
    sizes = np.full(k, CHUNK, np.int64)
    offs = np.arange(k, dtype=np.int64) * CHUNK
    dc = L.DeviceCodec("zstd", N, CHUNK, LEVEL)
    rc = L.RaggedCodec("zstd", CHUNK, k, LEVEL, max_total_bytes=N)
    out = torch.zeros(N + 256, dtype=torch.uint8, device="cuda")
    d_src, _ = rc._arrays(d_in, offs, sizes, 16)
    d_dst, _ = rc._arrays(out, offs, sizes, 0)
    res = dict(n=N, chunk=CHUNK, level=LEVEL, runs=RUNS, corpus="mixed seed 1",
               ragged_compress_temp=int(rc.ctemp.numel()), uniform_compress_temp=int(dc.ctemp.numel()),
               ragged_decompress_temp=int(rc.dtemp.numel()), uniform_decompress_temp=int(dc.dtemp.numel()))

    # compression: like for like = the uniform launcher's plain loop (no side-stream split)
    lib.lzh_debug_zstdc_split(0)
    res["compress_uniform_plain_a"] = timed(lambda: dc.compress(d_in))
    res["compress_ragged"] = timed(lambda: rc.compress_arrays(d_src, k))
    res["compress_uniform_plain_b"] = timed(lambda: dc.compress(d_in))
    lib.lzh_debug_zstdc_split(1)
    res["compress_uniform_default"] = timed(lambda: dc.compress(d_in))
    torch.cuda.synchronize()
    total = dc.packed_total()
    same = (rc.packed_total() == total and torch.equal(rc.csizes[:k], dc.csizes)
            and torch.equal(rc.offsets[: k + 1], dc.offsets) and torch.equal(rc.packed[:total], dc.packed[:total]))
    res["compress_same_bytes"] = bool(same)
    res["packed_total"] = int(total)

    # decompression: like for like = the uniform call's one-wave decoder
    lib.lzh_debug_zstd_legacy(1)
    res["decompress_uniform_onewave_a"] = timed(lambda: dc.decompress())
    res["decompress_ragged"] = timed(lambda: rc.decompress_arrays(d_dst, k))
    res["decompress_uniform_onewave_b"] = timed(lambda: dc.decompress())
    lib.lzh_debug_zstd_legacy(0)
    res["decompress_uniform_default"] = timed(lambda: dc.decompress())
    torch.cuda.synchronize()
    ok = (bool((rc.status[:k] == CHUNK).all()) and bool((dc.status == CHUNK).all())
          and torch.equal(out[:N], d_in[:N]) and torch.equal(dc.out[:N], d_in[:N]))
    res["decompress_same_bytes"] = bool(ok)

    # split decode: like for like = the uniform call's four-kernel decoder with every kernel on the caller's stream
    rs = L.RaggedCodec("zstd", CHUNK, k, LEVEL, max_total_bytes=N, split_decode=True)
    res["ragged_split_decompress_temp"] = int(rs.dtemp.numel())
    assert rs.dtemp.numel() == lib.lzh_zstd_ragged_decompress_split_temp_bytes(CHUNK, k) > rc.dtemp.numel()
    out.zero_()
    split = lambda: rs.decompress_arrays(d_dst, k, packed=rc.packed, csizes=rc.csizes, offsets=rc.offsets)  # noqa: E731
    lib.lzh_debug_zstd_side(0)
    res["split_uniform_one_stream_a"] = timed(lambda: dc.decompress())
    res["split_ragged"] = timed(split)
    res["split_uniform_one_stream_b"] = timed(lambda: dc.decompress())
    lib.lzh_debug_zstd_side(1)
    torch.cuda.synchronize()
    ok2 = bool((rs.status[:k] == CHUNK).all()) and torch.equal(out[:N], d_in[:N])
    res["split_ragged_onewave"] = timed(lambda: rc.decompress_arrays(d_dst, k))
    res["split_uniform_default"] = timed(lambda: dc.decompress())
    v = np.zeros(16, np.uint64)
    assert lib.lzh_debug_zstd_ragged_split_layout(CHUNK, k, v.ctypes.data) == 0
    split()
    torch.cuda.synchronize()
    st = rs.dtemp[int(v[6]): int(v[6]) + 4 * k].cpu().numpy().view(np.int32)
    res["split_frames_by_state"] = {str(int(a)): int(b) for a, b in zip(*np.unique(st, return_counts=True))}
    res["split_same_bytes"] = ok2
    ok = ok and ok2
    with open(os.path.join(OUT, "zstd_ragged_perf.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    assert same and ok


if __name__ == "__main__":
    main()
