"""tools/zstd_dict_perf.py [OUT.json] -- the zstd dictionary calls (include/lzbench_hip.h 3f) next to the plain ragged
zstd calls (3c) on the same device-resident records in one process: 4,096 JSON records of 1 KiB and of 16 KiB with a
64 KiB dictionary of the same corpus, levels 1 and -3.  Per case and level:
  dict_compress     lzh_zstd_compress_ragged_dict_async: zero + table kernels, match, entropy, scan, pack
  dict_tables       the same call on a batch of one empty chunk: the zero and table kernels and four near-empty
                    launches -- what a call pays once, whatever the batch
  dict_decompress   lzh_zstd_decompress_ragged_dict_async
  plain_compress / plain_decompress    lzh_zstd_compress_ragged_async / lzh_zstd_decompress_ragged_async (one-wave)
and the packed bytes of both.  The plain calls' kernels are the parent commit's, code hash for code hash
(tests/test_ragged_abi.py).  HIP events around each call, 3 warm-up and 20 timed rounds, all variants alternating inside
every round; medians with their range.  Both decoders' outputs are compared with the input."""
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
DICT = 65536


def measure(k, rec, level):
    n = k * rec
    host = L.datagen("json", DICT + n, seed=4242)
    d_all = torch.zeros(DICT + n + 256, dtype=torch.uint8, device="cuda")
    d_all[: DICT + n].copy_(torch.from_numpy(host))
    dictionary, d_in = d_all[:DICT], d_all[DICT:]
    offs, sizes = np.arange(k, dtype=np.int64) * rec, np.full(k, rec, np.int64)
    out = {v: torch.zeros(n + 256, dtype=torch.uint8, device="cuda") for v in ("dict", "plain")}
    rc = {"dict": L.RaggedCodec("zstd", rec, k, level, dictionary=dictionary), "plain": L.RaggedCodec("zstd", rec, k, level)}
    one = L.RaggedCodec("zstd", rec, 1, level, dictionary=dictionary)
    src = {v: rc[v]._arrays(d_in, offs, sizes, 16)[0] for v in rc}
    dst = {v: rc[v]._arrays(out[v], offs, sizes, 0)[0] for v in rc}
    empty = one._arrays(d_in, [0], [0], 16)[0]
    runs = {"dict_tables": (lambda: one.compress_arrays(empty, 1), 0)}
    for v in rc:
        runs[f"{v}_compress"] = (lambda v=v: rc[v].compress_arrays(src[v], k), n)
        runs[f"{v}_decompress"] = (lambda v=v: rc[v].decompress_arrays(dst[v], k), n)
    t = alternate({key: fn for key, (fn, _) in runs.items()}, WARM, REP)
    torch.cuda.synchronize()
    res = {"records": k, "record_bytes": rec, "dict_bytes": DICT, "level": level, "input_bytes": n, "warmup": WARM,
           "repeats": REP}
    for key, (_, nb) in runs.items():
        res[key] = stats(t[key], nb)
    for v in rc:
        assert torch.equal(out[v][:n], d_in[:n]), v
        assert bool((rc[v].status[:k] == rec).all()), v
        res[f"{v}_packed_bytes"] = rc[v].packed_total()
        res[f"{v}_compress_temp_bytes"] = rc[v].ctemp.numel()
    res["dict_over_plain_compress"] = res["dict_compress"]["median_ms"] / res["plain_compress"]["median_ms"]
    res["dict_over_plain_decompress"] = res["dict_decompress"]["median_ms"] / res["plain_decompress"]["median_ms"]
    res["dict_over_plain_packed"] = res["dict_packed_bytes"] / res["plain_packed_bytes"]
    return res


def main():
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0)}
    for rec in (1024, 16384):
        for level in (1, -3):
            name = f"json-4096x{rec // 1024}KiB-level{level}"
            out[name] = measure(4096, rec, level)
            print(name, json.dumps(out[name]), flush=True)
            torch.cuda.empty_cache()
            if len(sys.argv) > 1:
                with open(sys.argv[1], "w") as f:
                    json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
