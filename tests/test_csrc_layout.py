"""Layout of lzbench_amd/csrc: the decoders' shared device code is in headers (decode_win.h, zstdd.h), and the
switches retired with that move stay out.  Reads the sources only.

The ragged split decoder is the exception for now: zstd_ragged_split_hip.hip is the file it was, still includes
decode_hip.hip under LZH_DEVICE_FUNCTIONS_ONLY and keeps its own LZH_ZSTD_MINW block; the split decoder's device code
stays in decode_hip.hip until that unit moves (profiles/decode_headers/README.md)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lzbench_amd", "csrc")
SPLIT_UNIT = "zstd_ragged_split_hip.hip"


def _sources():
    return {f: open(os.path.join(CSRC, f), encoding="utf-8", errors="replace").read()
            for f in sorted(os.listdir(CSRC)) if f == "Makefile" or f.endswith((".hip", ".h", ".inc", ".cpp", ".c"))}


def _defining(name, empty=False):
    pat = r"^\s*#\s*define\s+%s\b" % name + (r"\s*(//.*)?$" if empty else "")
    return [f for f, s in _sources().items() if re.search(pat, s, re.M)]


def test_no_other_unit_includes_decode_hip():
    assert [f for f, s in _sources().items() if '#include "decode_hip.hip"' in s] == [SPLIT_UNIT]


def test_header_consumers_know_no_include_mode():
    src = _sources()
    for f in ("decode_win.h", "zstdd.h", "zstd_ragged_decode_hip.hip"):
        assert "LZH_DEVICE_FUNCTIONS_ONLY" not in src[f], f
    assert '#include "zstdd.h"' in src["zstd_dict_hip.hip"]


def test_zstd_minw_defined_in_the_header():
    assert sorted(_defining("LZH_ZSTD_MINW")) == sorted(["zstdd.h", SPLIT_UNIT])


def test_only_decode_hip_makes_the_header_tables_external():
    assert _defining("LZH_HDR_VAR", empty=True) == ["decode_hip.hip"]
    assert sorted(_defining("LZH_HDR_VAR")) == ["decode_hip.hip", "decode_win.h"]


def test_retired_switches_stay_out():
    for f, s in _sources().items():
        for name in ("LZH_DEC_RING", "LZH_ZSTD_PREF", "LZH_ZSTD_TAB17"):
            assert name not in s, (f, name)
