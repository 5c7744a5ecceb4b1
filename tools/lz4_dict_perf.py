"""tools/lz4_dict_perf.py [OUT.json] -- the LZ4 dictionary calls against the plain ragged LZ4 calls on one batch:
4096 chunks of 4 KiB JSON, a 64 KiB dictionary of the same corpus.  HIP events around each call, 5 warm-up and 30
timed rounds, the two variants alternating inside every round; medians with their range, and both packed sizes."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lzbench_amd as L  # noqa: E402
from perf_rounds import alternate  # noqa: E402

K, N, WARM, REP = 4096, 4096, 5, 30


def main():
    torch.cuda.set_device(0)
    d = L.datagen("json", 65536, seed=41)
    host = L.datagen("json", K * N + 64, seed=99)
    d_in = torch.from_numpy(host).cuda()
    offs, sizes = np.arange(K, dtype=np.int64) * N, np.full(K, N, np.int64)
    out = torch.zeros(K * N + 64, dtype=torch.uint8, device="cuda")
    codecs = (("plain", L.RaggedCodec("lz4", N, K)), ("dict", L.RaggedCodec("lz4", N, K, dictionary=torch.from_numpy(d))))
    arr = {name: (rc._arrays(d_in, offs, sizes, 16), rc._arrays(out, offs, sizes, 0)) for name, rc in codecs}
    torch.cuda.synchronize()
    runs = {}
    for name, rc in codecs:
        (src, k), (dst, _) = arr[name]
        runs[(name, "compress")] = lambda rc=rc, src=src, k=k: rc.compress_arrays(src, k)
        runs[(name, "decompress")] = lambda rc=rc, dst=dst, k=k: rc.decompress_arrays(dst, k)
    t = alternate(runs, WARM, REP)
    res = {"chunks": K, "chunk_bytes": N, "dict_bytes": len(d), "warmup": WARM, "repeats": REP, "input_bytes": K * N}
    for name, rc in codecs:
        assert (rc.status[:K].cpu().numpy() == N).all()
        res[name] = {"packed_bytes": rc.packed_total()}
        for w in ("compress", "decompress"):
            v = np.array(t[(name, w)])
            res[name][w + "_ms"] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
    assert (out[: K * N].cpu().numpy() == host[: K * N]).all()
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
