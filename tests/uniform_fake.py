"""The four uniform compress calls (lzh_compress_async, lzh_compress_kernel_stage, lzh_compress_kernel_only,
lzh_compress_finish_async) with made-up device pointers, for the CPU test of their argument checks
(tests/test_uniform_calls_abi.py), and the table of cases that test walks.

A case is a call, a codec and one or two defects put on an otherwise good set of arguments; two at once fix the order
of their checks.  The table holds only cases the call refuses (or, for the memcpy codec's empty input, answers) before
its first device call: a defect the call does not look at (lzh_compress_finish_async takes any d_in and in_readable,
the memcpy codec any temp) is in the table only beside one it does refuse.  The verdicts are not written by hand:

    LZH_LIB=<liblzbench_hip.so of the commit to be pinned> python tests/uniform_fake.py

records them as tests/golden/uniform_call_verdicts.json: {call: {codec number: {case name: return code}}}.
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lzbench_amd as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "uniform_call_verdicts.json")
OK, EARG, EHIP, ESPACE = 0, -1, -2, -3     # (include/lzbench_hip.h)
FAKE = 0x10000                              # a non-null "device pointer"
MIB = 1 << 20
LZ4, SNAPPY, MEMCPY, ZSTD = L.LZH_CODEC_LZ4, L.LZH_CODEC_SNAPPY, L.LZH_CODEC_MEMCPY, L.LZH_CODEC_ZSTD
LZ4F, NVLZ4, DFAST = L.LZH_CODEC_LZ4F, L.LZH_CODEC_NVLZ4, L.LZH_CODEC_ZSTD_DFAST
CODECS = (LZ4, SNAPPY, MEMCPY, ZSTD, LZ4F, NVLZ4, DFAST)
GOOD_LEVEL = {LZ4: 1, SNAPPY: 0, MEMCPY: 0, ZSTD: 1, LZ4F: 0, NVLZ4: 0, DFAST: 3}

# call -> (its pointers in the order of the C declaration, the ones it refuses when null)
CALLS = {
    "lzh_compress_async": (("d_in", "d_packed", "d_csizes", "d_offsets", "d_temp"),
                           ("d_in", "d_packed", "d_csizes", "d_offsets", "d_temp")),
    "lzh_compress_kernel_stage": (("d_in", "d_stage", "d_csizes"), ("d_in", "d_stage", "d_csizes")),
    "lzh_compress_kernel_only": (("d_in", "d_stage", "d_csizes"), ("d_in", "d_stage", "d_csizes")),
    "lzh_compress_finish_async": (("d_in", "d_stage", "d_csizes", "d_packed", "d_offsets"),
                                  ("d_stage", "d_csizes", "d_packed", "d_offsets")),
}
ASYNC, STAGE, ONLY, FINISH = CALLS

# defect -> the arguments it sets; a function: of the case's own n and of the sizing answers for its geometry
DEFECTS = {
    "chunk0": dict(chunk_size=0),
    "short_readable": dict(in_readable=lambda n, need, cap: n - 1),
    "level0": dict(level=0), "level19": dict(level=19),                 # zstd
    "level1": dict(level=1),                                            # the level-3 codec
    "bad_block_id": dict(level=1),                                      # LZ4F: block-size field 1 (4 .. 7 or 0)
    "level6": dict(level=6),                                            # the nvcomp container: 0 .. 5
    "chunk_over_16m": dict(chunk_size=16 * MIB + 1, n=2 * (16 * MIB + 1)),
    "chunks_over_u32": dict(chunk_size=1, n=1 << 32),
    "chunk_over_limit": dict(chunk_size=0x7fff0001, n=0x7fff0001),
    "temp_short": dict(temp_bytes=lambda n, need, cap: need - 1),
    "temp_null": dict(d_temp=None),
    "cap_short": dict(packed_cap=lambda n, need, cap: cap - 1),
}
LEVEL_DEFECTS = {ZSTD: ("level0", "level19"), DFAST: ("level1",), LZ4F: ("bad_block_id",), NVLZ4: ("level6",)}


def defects_of(call, codec):
    """{defect: whether the call refuses it on its own} for the defects that apply to (call, codec)"""
    pointers, required = CALLS[call]
    d = {"null_" + p: p in required for p in pointers if p != "d_temp"}
    d["chunk0"] = True
    d["short_readable"] = call == ASYNC
    takes = call != FINISH and codec != MEMCPY      # (the level, the u32 ranges: looked at by the codecs' paths)
    if call != FINISH:
        for name in LEVEL_DEFECTS.get(codec, ()):
            d[name] = True
    if codec == DFAST:
        d["chunk_over_16m"] = takes
    d["chunks_over_u32"] = d["chunk_over_limit"] = takes
    if call == ASYNC:
        d["temp_short"] = d["temp_null"] = codec != MEMCPY
    if call in (ASYNC, FINISH):
        d["cap_short"] = True
    return d


def always_refused(call, codec):
    """the call takes this codec with no arguments at all"""
    if call == FINISH:
        return codec not in (LZ4, SNAPPY, ZSTD)
    if call == ASYNC:
        return False
    return codec in (MEMCPY, DFAST) or (call == ONLY and codec in (LZ4F, NVLZ4))


def settings(name):
    return {"d_" + name[7:]: None} if name.startswith("null_d_") else DEFECTS[name]


def cases(call, codec):
    """{case name: the defects of the case}: every defect alone and every pair that can stand together, where the call
    returns before its first device call; for the memcpy codec its two LZH_OK answers as well."""
    d = defects_of(call, codec)
    out = {}
    if always_refused(call, codec):
        out["good"] = ()
    for k in (1, 2):
        for combo in itertools.combinations(d, k):
            keys = [key for name in combo for key in settings(name)]
            if len(keys) != len(set(keys)):
                continue                    # (two values for one argument)
            if always_refused(call, codec) or any(d[name] for name in combo):
                out["+".join(combo)] = combo
    if call == ASYNC and codec == MEMCPY:
        out["empty"] = out["empty+null_d_in+temp_null"] = None     # (filled in by arguments())
    return out


def arguments(call, codec, name, combo):
    lib = L.lib()
    v = dict(codec=codec, level=GOOD_LEVEL[codec], stage_mask=3, n=3 * 131072 + 1, chunk_size=131072, stream=None,
             temp_bytes=lambda n, need, cap: need, packed_cap=lambda n, need, cap: cap,
             in_readable=lambda n, need, cap: n + 64, **{p: FAKE for p in CALLS[call][0]})
    if combo is None:
        v.update(n=0)
        if "+" in name:
            v.update(d_in=None, d_temp=None, temp_bytes=0)
    for defect in combo or ():
        v.update(settings(defect))
    # (the sizing calls divide by the chunk size: the call refuses a zero before it asks them)
    chunk = v["chunk_size"] or 131072
    need = lib.lzh_compress_temp_bytes(codec, v["n"], chunk)
    cap = v["n"] if codec == MEMCPY else lib.lzh_max_packed_bytes(codec, v["n"], chunk)
    return {key: x(v["n"], need, cap) if callable(x) else x for key, x in v.items()}


ORDER = {
    ASYNC: ("codec", "level", "d_in", "n", "in_readable", "chunk_size", "d_packed", "packed_cap", "d_csizes", "d_offsets",
            "d_temp", "temp_bytes", "stream"),
    STAGE: ("codec", "level", "stage_mask", "d_in", "n", "in_readable", "chunk_size", "d_stage", "d_csizes", "stream"),
    ONLY: ("codec", "level", "d_in", "n", "in_readable", "chunk_size", "d_stage", "d_csizes", "stream"),
    FINISH: ("codec", "d_in", "n", "in_readable", "chunk_size", "d_stage", "d_csizes", "d_packed", "packed_cap", "d_offsets",
             "stream"),
}


def fake_call(call, codec, name, combo):
    v = arguments(call, codec, name, combo)
    return getattr(L.lib(), call)(*(v[a] for a in ORDER[call]))


def main():
    table = {}
    for call in CALLS:
        for codec in CODECS:
            t = table.setdefault(call, {})[str(codec)] = {}
            for name, combo in cases(call, codec).items():
                rc = fake_call(call, codec, name, combo)
                # LZH_EHIP: the case reached a device call, which has no device here -- a mistake of defects_of()
                assert rc in (OK, EARG, ESPACE) and (rc != OK or combo is None), (call, codec, name, rc)
                t[name] = rc
    with open(GOLDEN, "w") as f:
        json.dump(table, f, sort_keys=True, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"{GOLDEN}: {sum(len(t) for c in table.values() for t in c.values())} verdicts of {L.LIB_PATH}")


if __name__ == "__main__":
    main()
