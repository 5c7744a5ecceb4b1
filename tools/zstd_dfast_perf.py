"""tools/zstd_dfast_perf.py [OUT.json] -- zstd level 3 (zstd_dfast, LZH_CODEC_ZSTD_DFAST) next to zstd level 1 on the
same device-resident input in the same run: 4096 x 128 KiB chunks of `mixed`, and 1 GiB of `text` at -b1024.  HIP
events around each compress call, 3 warm-up and 30 timed rounds, the two codecs alternating inside every round;
medians with their range and both packed sizes.  The CPU row is the reference build's zstd -3 on one thread, by
bench.py's CPU-baseline method (best of 3 passes over a 64 MiB sample of the same corpus); without the reference
build it is left out."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lzbench_amd as L  # noqa: E402
from perf_rounds import alternate  # noqa: E402

WARM, REP = 3, 30
WORKLOADS = (("mixed-4096x128KiB", "mixed", 4096 * 131072, 131072), ("text-1GiB-b1024", "text", 1 << 30, 1 << 20))


def cpu_row(host, chunk):
    import bench
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    if not O.have_ref():
        return None
    r = bench.cpu_baseline(host[:64 << 20], "zstd", chunk, 3, 3, 0)
    return {"comp_MBps": r["comp_MBps"], "decomp_MBps": r["decomp_MBps"], "roundtrip_ok": r["roundtrip_ok"], "sample": r["sample"]}


def measure(name, kind, n, chunk):
    host = L.datagen(kind, n, seed=12345)
    d_in = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(torch.from_numpy(host))
    res = {"corpus": kind, "input_bytes": n, "chunk_bytes": chunk, "warmup": WARM, "repeats": REP}
    codecs = (("zstd_level1", "zstd", 1), ("zstd_dfast_level3", "zstd_dfast", 3))
    dcs = {}
    for key, codec, level in codecs:
        dcs[key] = L.DeviceCodec(codec, n, chunk, level=level)
    t = alternate({key: lambda key=key: dcs[key].compress(d_in) for key, _, _ in codecs}, WARM, REP)
    for key, _, _ in codecs:
        dc = dcs[key]
        dc.decompress()
        torch.cuda.synchronize()
        assert (dc.status.cpu().numpy() >= 0).all() and torch.equal(dc.out[:n], d_in[:n]), key
        v = np.array(t[key])
        res[key] = {"packed_bytes": dc.packed_total(),
                    "compress_ms": {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())},
                    "compress_GBps": n / float(np.median(v)) / 1e6}
    res["level3_over_level1_time"] = res["zstd_dfast_level3"]["compress_ms"]["median"] / res["zstd_level1"]["compress_ms"]["median"]
    del dcs, d_in
    torch.cuda.empty_cache()
    cpu = cpu_row(host, chunk)
    if cpu:
        res["cpu_zstd_level3_one_thread"] = cpu
    return name, res


def main():
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0)}
    for w in WORKLOADS:
        name, res = measure(*w)
        out[name] = res
        print(name, json.dumps(res), flush=True)
        if len(sys.argv) > 1:
            with open(sys.argv[1], "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
