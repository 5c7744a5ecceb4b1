"""tools/zstd_dfast_ragged_perf.py [OUT.json] -- the ragged zstd calls at level 3 (include/lzbench_hip.h 3e) and at
level 1 (3c) next to the uniform call, on the same device-resident input in one process:
  mixed-4096x128KiB   4096 equal chunks of `mixed` through the uniform call (DeviceCodec), the ragged uniform-slot call
                      and the ragged compact call;
  json-65536x4KiB     65,536 records of 4 KiB of `json` through the two ragged calls, and the time of zeroing as many
                      bytes as the level-3 frames' tables hold (48 KiB a record) with one device memset: a lower
                      bound of what the per-frame zeroing costs inside the match kernel, not a measurement of it.
HIP events around each compress call, 3 warm-up and 20 timed rounds, all variants alternating inside every round;
medians with their range, so a ragged call's gap to the uniform call reads against the uniform call's own spread.
Every variant's packed output is compared with the first one's of its level."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lzbench_amd as L  # noqa: E402
from perf_rounds import alternate, stats, timed  # noqa: E402

WARM, REP = 3, 20
LEVELS = (("level3", "zstd_dfast", 3), ("level1", "zstd", 1))


def measure(kind, k, chunk, uniform):
    n = k * chunk
    host = L.datagen(kind, n, seed=12345)
    d_in = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(torch.from_numpy(host))
    offs, sizes = np.arange(k, dtype=np.int64) * chunk, np.full(k, chunk, np.int64)
    res = {"corpus": kind, "chunks": k, "chunk_bytes": chunk, "input_bytes": n, "warmup": WARM, "repeats": REP}
    runs = {}
    for lname, codec, level in LEVELS:
        if uniform:
            dc = L.DeviceCodec(codec, n, chunk, level=level)
            runs[f"{lname}_uniform_call"] = (dc, lambda dc=dc: dc.compress(d_in), dc.ctemp.numel() if hasattr(dc, "ctemp") else None)
        for vname, compact in (("ragged_uniform_slots", False), ("ragged_compact", True)):
            rc = L.RaggedCodec(codec, chunk, k, level, max_total_bytes=n, compact_scratch=compact)
            d, _ = rc._arrays(d_in, offs, sizes, 16)
            runs[f"{lname}_{vname}"] = (rc, lambda rc=rc, d=d: rc.compress_arrays(d, k), rc.ctemp.numel())
    t = alternate({key: fn for key, (_, fn, _) in runs.items()}, WARM, REP)
    torch.cuda.synchronize()
    first = {}
    for key, (c, _, temp) in runs.items():
        total = c.packed_total()
        lname = key.split("_")[0]
        if lname not in first:
            first[lname] = c.packed[:total].clone()
        assert total == first[lname].numel() and torch.equal(c.packed[:total], first[lname]), key
        res[key] = dict(stats(t[key], n), packed_bytes=total, temp_bytes=temp)
    for lname, _, _ in LEVELS:
        base = f"{lname}_uniform_call" if uniform else f"{lname}_ragged_uniform_slots"
        for vname in ("ragged_uniform_slots", "ragged_compact"):
            if f"{lname}_{vname}" != base:
                res[f"{lname}_{vname}_over_{base.split('_', 1)[1]}"] = res[f"{lname}_{vname}"]["median_ms"] / res[base]["median_ms"]
    if not uniform:   # the level-3 tables of the batch, zeroed once by a device memset
        tab = torch.empty(k * (48 << 10), dtype=torch.uint8, device="cuda")
        v = [timed(lambda: tab.zero_()) for _ in range(WARM + REP)][WARM:]
        res["memset_of_the_level3_tables"] = dict(stats(v, tab.numel()), bytes=tab.numel())
        res["memset_share_of_level3_ragged_uniform_slots"] = (res["memset_of_the_level3_tables"]["median_ms"]
                                                              / res["level3_ragged_uniform_slots"]["median_ms"])
    return res


def main():
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0)}
    for name, args in (("mixed-4096x128KiB", ("mixed", 4096, 131072, True)), ("json-65536x4KiB", ("json", 65536, 4096, False))):
        out[name] = measure(*args)
        print(name, json.dumps(out[name]), flush=True)
        torch.cuda.empty_cache()
        if len(sys.argv) > 1:
            with open(sys.argv[1], "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
