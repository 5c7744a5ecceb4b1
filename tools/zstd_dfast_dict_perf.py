"""tools/zstd_dfast_dict_perf.py [OUT.json] -- the zstd level-3 dictionary call (include/lzbench_hip.h 3h) next to
3f's level-1 dictionary call and the plain level-3 ragged call (3e) on the same device-resident records in one
process: 4,096 JSON records of 1 KiB and of 16 KiB with a 64 KiB dictionary of the same corpus.  Per case:
  dfast_dict_compress   lzh_zstd_dfast_compress_ragged_dict_async: zero + table kernels, match, entropy, scan, pack
  dfast_dict_tables     the same call on a batch of one empty chunk: what a call pays once, whatever the batch
  dict1_compress        lzh_zstd_compress_ragged_dict_async at level 1
  plain3_compress       lzh_zstd_dfast_compress_ragged_async (level 3, no dictionary)
  dfast_dict_decompress / dict1_decompress    lzh_zstd_decompress_ragged_dict_async on either call's frames
and the packed and temp bytes of all three; where the reference build is there, what ZSTD_compress_usingDict writes at
level 3 for the same records, which must be the same number of bytes.  The two older calls' kernels are the parent
commit's, code hash for code hash (tests/test_ragged_abi.py).  HIP events around each call, 3 warm-up and 20 timed
rounds, all variants alternating inside every round; medians with their range.  The decoders' outputs are compared
with the input."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lzbench_amd as L  # noqa: E402
from perf_rounds import alternate, stats  # noqa: E402

WARM, REP = 3, 20
DICT = 65536


def reference_bytes(host, k, rec):
    """the bytes ZSTD_compress_usingDict writes at level 3 for the k records, raw-store rule applied; None without
    the reference build"""
    try:
        import zstd_dict_ref as R
        if R.missing():
            return None
    except Exception:
        return None
    d = host[:DICT]
    return sum(len(R.packed(d, host[DICT + i * rec: DICT + (i + 1) * rec], 3)) for i in range(k))


def measure(k, rec):
    n = k * rec
    host = L.datagen("json", DICT + n, seed=4242)
    d_all = torch.zeros(DICT + n + 256, dtype=torch.uint8, device="cuda")
    d_all[: DICT + n].copy_(torch.from_numpy(host))
    dictionary, d_in = d_all[:DICT], d_all[DICT:]
    offs, sizes = np.arange(k, dtype=np.int64) * rec, np.full(k, rec, np.int64)
    rc = {"dfast_dict": L.RaggedCodec("zstd_dfast_dict", rec, k, 3, dictionary=dictionary),
          "dict1": L.RaggedCodec("zstd", rec, k, 1, dictionary=dictionary),
          "plain3": L.RaggedCodec("zstd_dfast", rec, k, 3)}
    out = {v: torch.zeros(n + 256, dtype=torch.uint8, device="cuda") for v in rc}
    one = L.RaggedCodec("zstd_dfast_dict", rec, 1, 3, dictionary=dictionary)
    src = {v: rc[v]._arrays(d_in, offs, sizes, 16)[0] for v in rc}
    dst = {v: rc[v]._arrays(out[v], offs, sizes, 0)[0] for v in rc}
    empty = one._arrays(d_in, [0], [0], 16)[0]
    runs = {"dfast_dict_tables": (lambda: one.compress_arrays(empty, 1), 0)}
    for v in rc:
        runs[f"{v}_compress"] = (lambda v=v: rc[v].compress_arrays(src[v], k), n)
        runs[f"{v}_decompress"] = (lambda v=v: rc[v].decompress_arrays(dst[v], k), n)
    t = alternate({key: fn for key, (fn, _) in runs.items()}, WARM, REP)
    torch.cuda.synchronize()
    res = {"records": k, "record_bytes": rec, "dict_bytes": DICT, "input_bytes": n, "warmup": WARM, "repeats": REP}
    for key, (_, nb) in runs.items():
        res[key] = stats(t[key], nb)
    for v in rc:
        assert torch.equal(out[v][:n], d_in[:n]), v
        assert bool((rc[v].status[:k] == rec).all()), v
        res[f"{v}_packed_bytes"] = rc[v].packed_total()
        res[f"{v}_compress_temp_bytes"] = rc[v].ctemp.numel()
    ref = reference_bytes(host, k, rec)
    res["reference_level3_dict_packed_bytes"] = ref
    assert ref is None or ref == res["dfast_dict_packed_bytes"], (ref, res["dfast_dict_packed_bytes"])
    res["dfast_dict_over_dict1_compress"] = res["dfast_dict_compress"]["median_ms"] / res["dict1_compress"]["median_ms"]
    res["dfast_dict_over_plain3_compress"] = res["dfast_dict_compress"]["median_ms"] / res["plain3_compress"]["median_ms"]
    res["dfast_dict_over_dict1_packed"] = res["dfast_dict_packed_bytes"] / res["dict1_packed_bytes"]
    res["dfast_dict_over_plain3_packed"] = res["dfast_dict_packed_bytes"] / res["plain3_packed_bytes"]
    return res


def main():
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "tables": "a zeroed private pair per frame over the class's shared filled pair"}
    for rec in (1024, 16384):
        name = f"json-4096x{rec // 1024}KiB"
        out[name] = measure(4096, rec)
        print(name, json.dumps(out[name]), flush=True)
        torch.cuda.empty_cache()
        if len(sys.argv) > 1:
            with open(sys.argv[1], "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
