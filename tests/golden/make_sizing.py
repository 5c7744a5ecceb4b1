#!/usr/bin/env python3
"""tests/golden/make_sizing.py -- the answers of every sizing entry point of the device API over a fixed grid.

The temp layouts of lzbench_amd/csrc are laid out once per buffer and read by the sizing call and by the launch;
sizing.json pins what the sizing calls returned before that was so, for tests/test_sizing_golden.py.  Pure host
arithmetic: needs the built liblzbench_hip.so, no GPU and no reference build.  Run on the commit whose answers are
to be pinned (python tests/golden/make_sizing.py); LZH_LIB names another build of the library.

Writes sizing.json, for the ragged zstd calls sizing_zstd_ragged.json and for their compact layout
sizing_zstd_ragged_compact.json, each {"grid": {...}, "tables":
{function: {codec number: [values in the grid's loop order]}}, "sha256": digest of the tables}.  Loop order: the arguments in the order of the C declaration, the first one
outermost.  lzh_debug_ragged_compact_regions gives four values per point; lzh_debug_plan gives, per point, its
return value and then that many values.  The ragged zstd calls (levels 1 and -1 where they take one, over
chunk x nchunks) have one list each, under codec "3"; lzh_debug_zstd_ragged_split_layout gives its 16 values per
point, or its error code 16 times.  The two compact ones (levels 1 and -1 over n x chunk x nchunks, n the batch's
total bytes): lzh_debug_zstd_ragged_compact_regions gives four values per point, or its error code four times.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

MiB = 1 << 20
GRID = {
    "codecs": [0, 1, 2, 3, 4, 5],
    "n": [0, 1, 4095, 4096, 65535, 65536, 65537, 200000, MiB, 16 * MiB + 1, 1 << 30],
    "chunk": [1, 4096, 65536, 65537, 131072, 131073, MiB, 16 * MiB, 16 * MiB + 1, 1 << 30],
    "nchunks": [0, 1, 2, 255, 256, 257, 1000, 16384],
    "shards": [1, 2, 8],
}


def tables(lib) -> dict:
    """{function: {codec: [values]}} of `lib` (lzbench_amd.lib()) over GRID."""
    N, CH, K, SH = GRID["n"], GRID["chunk"], GRID["nchunks"], GRID["shards"]
    out = {}

    def table(name, fn):
        out[name] = {str(c): [int(v) for v in fn(c)] for c in GRID["codecs"]}

    def regions(c):
        r = (C.c_uint64 * 4)()
        for t in N:
            for m in CH:
                for k in K:
                    rc = lib.lzh_debug_ragged_compact_regions(c, t, m, k, r)
                    yield from (list(r) if rc == 0 else [rc] * 4)

    def plan(c):
        v = (C.c_uint64 * 80)()
        for g in SH:
            for n in N:
                for ch in CH:
                    m = lib.lzh_debug_plan(g, n, ch, c, v, 80)
                    yield m
                    yield from v[:m]

    table("lzh_stage_stride", lambda c: (lib.lzh_stage_stride(c, ch) for ch in CH))
    for name in ("lzh_max_packed_bytes", "lzh_compress_temp_bytes", "lzh_decompress_temp_bytes"):
        table(name, lambda c, f=getattr(lib, name): (f(c, n, ch) for n in N for ch in CH))
    for name in ("lzh_ragged_compress_temp_bytes", "lzh_ragged_decompress_temp_bytes"):
        table(name, lambda c, f=getattr(lib, name): (f(c, m, k) for m in CH for k in K))
    table("lzh_ragged_max_packed_bytes", lambda c: (lib.lzh_ragged_max_packed_bytes(c, t, k) for t in N for k in K))
    table("lzh_ragged_compact_compress_temp_bytes",
          lambda c: (lib.lzh_ragged_compact_compress_temp_bytes(c, t, m, k) for t in N for m in CH for k in K))
    table("lzh_debug_ragged_compact_regions", regions)
    table("lzh_debug_plan", plan)

    # the ragged zstd calls take no codec: their tables are keyed under zstd's number alone
    def zstd_table(name, values):
        out[name] = {"3": [int(v) for v in values]}

    def split_layout():
        r = (C.c_uint64 * 16)()
        for m in CH:
            for k in K:
                rc = lib.lzh_debug_zstd_ragged_split_layout(m, k, r)
                yield from (list(r) if rc == 0 else [rc] * 16)

    zstd_table("lzh_zstd_ragged_compress_temp_bytes",
               (lib.lzh_zstd_ragged_compress_temp_bytes(lv, m, k) for lv in (1, -1) for m in CH for k in K))
    for name in ("lzh_zstd_ragged_decompress_temp_bytes", "lzh_zstd_ragged_decompress_split_temp_bytes",
                 "lzh_zstd_ragged_max_packed_bytes"):   # (the last one's first argument is the batch's total bytes)
        zstd_table(name, (getattr(lib, name)(m, k) for m in CH for k in K))
    zstd_table("lzh_debug_zstd_ragged_split_layout", split_layout())

    def zstd_regions():
        r = (C.c_uint64 * 4)()
        for lv in (1, -1):
            for t in N:
                for m in CH:
                    for k in K:
                        rc = lib.lzh_debug_zstd_ragged_compact_regions(lv, t, m, k, r)
                        yield from (list(r) if rc == 0 else [rc] * 4)

    zstd_table("lzh_zstd_ragged_compact_compress_temp_bytes",
               (lib.lzh_zstd_ragged_compact_compress_temp_bytes(lv, t, m, k)
                for lv in (1, -1) for t in N for m in CH for k in K))
    zstd_table("lzh_debug_zstd_ragged_compact_regions", zstd_regions())
    return out


def digest(tabs: dict) -> str:
    return hashlib.sha256(json.dumps(tabs, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def files(tabs: dict) -> dict:
    """{file name: its tables}: the ragged zstd tables have a file of their own, and those of their compact layout
    another, so that adding them left sizing.json, a single line of 190 KB, and then both files as they were."""
    compact = {name: t for name, t in tabs.items() if "zstd_ragged_compact" in name}
    own = {name: t for name, t in tabs.items() if "zstd_ragged" in name and name not in compact}
    return {"sizing.json": {name: t for name, t in tabs.items() if "zstd_ragged" not in name},
            "sizing_zstd_ragged.json": own, "sizing_zstd_ragged_compact.json": compact}


def main():
    import lzbench_amd as L
    for fname, tabs in files(tables(L.lib())).items():
        with open(os.path.join(HERE, fname), "w") as f:
            json.dump({"grid": GRID, "tables": tabs, "sha256": digest(tabs)}, f, sort_keys=True, separators=(",", ":"))
            f.write("\n")
        print(f"{fname}: {sum(len(v) for t in tabs.values() for v in t.values())} values, sha256 {digest(tabs)}")


if __name__ == "__main__":
    main()
