"""CPU: every sizing entry point of the device API answers what tests/golden/sizing*.json recorded (the temp layouts
of lzbench_amd/csrc/temp_layout.h give the sizes the hand-kept sums gave before them; sizing_zstd_ragged_compact.json
holds the compact zstd layout's sizes and regions from before it shared the LZ4 / snappy layout's struct), and the
ragged uniform-slot compress temp is the uniform call's for the same slots."""
import importlib.util
import json
import os

import lzbench_amd as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_sizing", os.path.join(GOLDEN, "make_sizing.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_sizing_answers_equal_the_recorded_ones():
    M = _maker()
    for fname, got in M.files(M.tables(L.lib())).items():   # (sizing.json, the ragged zstd calls' file, their compact layout's)
        with open(os.path.join(GOLDEN, fname)) as f:
            want = json.load(f)
        assert want["grid"] == M.GRID, f"{fname} was made over another grid"
        assert M.digest(want["tables"]) == want["sha256"], f"{fname} was edited by hand"
        assert got and sorted(got) == sorted(want["tables"])
        for name, per_codec in want["tables"].items():
            assert sorted(got[name]) == sorted(per_codec), name
            for codec, values in per_codec.items():
                have = got[name][codec]
                assert len(have) == len(values), (name, codec)
                bad = [(i, a, b) for i, (a, b) in enumerate(zip(have, values)) if a != b]
                assert not bad, f"{name}, codec {codec}: {len(bad)} answers changed, first (index, now, recorded) {bad[0]}"
        assert M.digest(got) == want["sha256"]


def test_ragged_uniform_slots_size_as_the_uniform_call():
    """k slots of m bytes are k chunks of m bytes: one layout serves both calls.  (Every point of the grid with
    m <= 16 MiB, k >= 1 holds on the commit before the shared layout: none is left out.)"""
    M = _maker()
    lib = L.lib()
    for codec in (L.LZH_CODEC_LZ4, L.LZH_CODEC_SNAPPY):
        for m in M.GRID["chunk"]:
            for k in M.GRID["nchunks"]:
                if m > 16 << 20 or k < 1:
                    continue
                assert lib.lzh_ragged_compress_temp_bytes(codec, m, k) == lib.lzh_compress_temp_bytes(codec, k * m, m), \
                    (codec, m, k)
