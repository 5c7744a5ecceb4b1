"""Layout of lzbench_amd/csrc: the decoders' shared device code is in headers (decode_win.h, zstdd.h), so is that of
the LZ4, snappy and zstd compressors (lz4c.h, snappyc.h, zstdc.h, zstdc_dfast.h), and the switches retired with the
first move stay out.  Reads the sources only; the one compile is a syntax check of each compressor header on its own
(and of the one include order that zstdc_dfast.h refuses).

The ragged split decoder is the exception for now: zstd_ragged_split_hip.hip is the file it was, still includes
decode_hip.hip under LZH_DEVICE_FUNCTIONS_ONLY and keeps its own LZH_ZSTD_MINW block; the split decoder's device code
stays in decode_hip.hip until that unit moves (profiles/decode_headers/README.md)."""
import os
import re
import subprocess

import pytest

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


# The compressors: device code in lz4c.h, snappyc.h, zstdc.h and zstdc_dfast.h (the level-3 codec: zstdc.h compiled
# for ZSTD_dfast, and namespace zdf), which the codecs' own units and the ragged, compact and dictionary units include.
COMPRESS_HEADERS = ("lz4c.h", "snappyc.h", "zstdc.h", "zstdc_dfast.h")
COMPRESS_UNITS = ("lz4c_hip.hip", "snappyc_hip.hip")
ZSTDC_UNITS = ("zstdc_hip.hip", "zstdc_dfast_hip.hip")
ZSTDC_CONSUMERS = ("zstd_ragged_hip.hip", "zstd_ragged_compact_hip.hip", "zstd_dict_hip.hip")   # (+ the dfast ragged unit)


def _syntax_check(tmp_path, text):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: cannot compile the header")
    unit = tmp_path / "first.hip"
    unit.write_text(text)
    return subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(unit)],
                          capture_output=True, text=True)


def test_no_unit_includes_the_lz4_or_snappy_compressor_file():
    for f, s in _sources().items():
        for unit in COMPRESS_UNITS:
            assert not re.search(r'#\s*include\s*"%s"' % re.escape(unit), s), (f, unit)


def test_no_unit_includes_a_zstd_compressor_file():
    for f, s in _sources().items():
        for unit in ZSTDC_UNITS:
            assert not re.search(r'#\s*include\s*"%s"' % re.escape(unit), s), (f, unit)


def test_include_modes_are_the_split_decoders_alone():
    """LZH_DEVICE_FUNCTIONS_ONLY is left in decode_hip.hip and the one unit that includes it; the level-3 codec's
    mode of its own is gone."""
    src = _sources()
    assert [f for f, s in src.items() if "LZH_DEVICE_FUNCTIONS_ONLY" in s.replace("LZH_DFAST_DEVICE_FUNCTIONS_ONLY", "")] \
        == ["decode_hip.hip", SPLIT_UNIT]
    assert [f for f, s in src.items() if "LZH_DFAST_DEVICE_FUNCTIONS_ONLY" in s] == []


def test_zstd_compress_units_include_the_headers():
    src = _sources()
    for f in ("zstdc_hip.hip",) + ZSTDC_CONSUMERS + ("zstdc_dfast.h",):
        assert '#include "zstdc.h"' in src[f], f
    for f in ("zstdc_dfast_hip.hip", "zstd_dfast_ragged_hip.hip"):
        assert '#include "zstdc_dfast.h"' in src[f], f
        assert '#include "zstdc.h"' not in src[f], f   # (through zstdc_dfast.h, which sets the strategy first)
    for h in ("zstdc.h", "zstdc_dfast.h"):
        assert "__global__" not in src[h], h
        code = [l for l in src[h].splitlines() if l.strip() and not l.lstrip().startswith("//")]
        assert code[0] == "#pragma once", h


def test_only_zstdc_hip_makes_the_compressor_tables_external():
    """LZH_TU_VAR, the LZH_HDR_VAR of the compressor's header: static in zstdc.h unless the unit defined it, and
    zstdc_hip.hip alone defines it empty; common.h no longer knows of it."""
    assert _defining("LZH_TU_VAR", empty=True) == ["zstdc_hip.hip"]
    assert sorted(_defining("LZH_TU_VAR")) == ["zstdc.h", "zstdc_hip.hip"]
    assert [f for f, s in _sources().items() if "LZH_TU_VAR" in s] == ["zstdc.h", "zstdc_hip.hip"]


def test_zstdc_after_its_default_strategy_is_an_error(tmp_path):
    """zstdc.h first and zstdc_dfast.h after it would compile the entropy stage for strategy 1 without a word."""
    r = _syntax_check(tmp_path, '#include "zstdc.h"\n#include "zstdc_dfast.h"\n')
    assert r.returncode != 0
    assert "zstdc_dfast.h must come before zstdc.h" in r.stderr


def test_compress_header_units_know_no_include_mode():
    src = _sources()
    for f in COMPRESS_UNITS + ZSTDC_UNITS + ("ragged_hip.hip", "ragged_compact_hip.hip", "lz4_dict_hip.hip") \
            + ZSTDC_CONSUMERS + ("zstd_dfast_ragged_hip.hip",) + COMPRESS_HEADERS:
        assert "LZH_DEVICE_FUNCTIONS_ONLY" not in src[f], f
    for f in ("lz4c_hip.hip", "ragged_hip.hip", "ragged_compact_hip.hip", "lz4_dict_hip.hip"):
        assert '#include "lz4c.h"' in src[f], f
    for f in ("snappyc_hip.hip", "ragged_hip.hip", "ragged_compact_hip.hip"):
        assert '#include "snappyc.h"' in src[f], f


def test_makefile_names_no_compressor_file_as_a_prerequisite():
    """The four files stand in the Makefile only as the sources of their own objects (the pattern rule)."""
    text = re.sub(r"\\\n", " ", _sources()["Makefile"])
    for line in text.splitlines():
        if line.startswith(("#", "\t")) or ":" not in line:
            continue
        target, _, prereq = line.partition(":")
        if prereq.startswith("="):   # (a `:=` assignment)
            continue
        for unit in COMPRESS_UNITS + ZSTDC_UNITS:
            assert unit not in prereq.split(), line


# The zstd dictionary compressors (levels 1 and 3): what stands around their two walks is zstd_dict_env.h, once.
DICT_ENV = "zstd_dict_env.h"


def test_both_dictionary_units_include_the_shared_environment():
    src = _sources()
    for f in ("zstd_dict_hip.hip", "zstd_dfast_dict_hip.hip"):
        assert '#include "%s"' % DICT_ENV in src[f], f
    assert "__global__" not in src[DICT_ENV]


def test_two_view_counts_are_defined_once():
    for name in ("count_fwd2", "count_bwd2"):
        assert [f for f, s in _sources().items() if re.search(r"^__device__ .*\b%s\(" % name, s, re.M)] == [DICT_ENV]


# The ragged compress calls: one batch struct and one slots struct per layout from api.cpp's ragged_compress to the
# launchers (launch.h LzhBatch, LzhSlots, LzhCompactSlots).
def _code(text):
    """the text without its // comments"""
    return re.sub(r"//[^\n]*", "", text)


def test_launch_h_names_the_batch_arrays_in_the_batch_struct_alone():
    code = _code(_sources()["launch.h"])
    assert re.search(r"struct LzhBatch \{\s*const void\* const\* ptrs;\s*const uint64_t\* bytes;", code)
    for name in ("in_ptrs", "in_bytes"):
        assert not re.search(r"\b%s\b" % name, code), name
    assert len(re.findall(r"\bconst void\* const\*", code)) == 1   # (the struct's field: no launcher spells it out)


def test_api_packs_and_tests_its_pointers_in_one_place():
    code = _code(_sources()["api.cpp"])
    for launcher in ("lzh_launch_pack_ragged(", "lzh_launch_pack_compact("):
        assert code.count(launcher) == 1, launcher
    six = r"d_in_ptrs\s*&&\s*d_in_bytes\s*&&\s*d_packed\s*&&\s*d_csizes\s*&&\s*d_offsets\s*&&\s*d_temp\b"
    assert len(re.findall(six, code)) == 1
    # (and no entry point tests a part of it on its own)
    assert len(re.findall(r"d_in_ptrs\s*&&", code)) == 1


# The uniform compress calls: the input struct and the slots of the call's layout from api.cpp's uniform_call to the
# launchers (launch.h LzhInput, LzhSlots, LzhFrameSlots).
def test_launch_h_names_the_input_in_the_input_struct_alone():
    code = _code(_sources()["launch.h"])
    assert re.search(r"struct LzhInput \{\s*const uint8_t\* in;\s*uint64_t n_total, in_readable, chunk_size;", code)
    assert len(re.findall(r"\bin_readable\b", code)) == 1
    assert len(re.findall(r"\bstruct \w*Slots \{", code)) == 3   # (LzhSlots, LzhFrameSlots, LzhCompactSlots)


def test_api_has_one_uniform_scan_and_pack_and_one_range_check():
    code = _code(_sources()["api.cpp"])
    for launcher in ("lzh_launch_pack(", "lzh_launch_frame_pack("):
        assert code.count(launcher) == 1, launcher
    assert code.count("0x7fff0000u") == 1
    # the layouts hand out the slots: no offset arithmetic in the compress calls
    uniform = code[code.index("static bool fits_u32("):code.index("int lzh_decompress_async(")]
    assert "lzh_compress_finish_async(" in uniform and not re.search(r"\bbase \+", uniform)
    for layout in ("chunk_temp(", "frame_temp(", "frame_geo("):
        assert uniform.count(layout) == 1, layout


@pytest.mark.parametrize("header", COMPRESS_HEADERS + (DICT_ENV,))
def test_compress_header_compiles_when_included_first(header, tmp_path):
    r = _syntax_check(tmp_path, '#include "%s"\n' % header)
    assert r.returncode == 0, r.stderr
