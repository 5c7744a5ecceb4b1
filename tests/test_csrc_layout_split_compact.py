"""Layout of lzbench_amd/csrc, the ragged split decoder's compact unit (include/lzbench_hip.h 3g).  test_csrc_layout.py
keeps zstd_ragged_split_hip.hip as the one file that includes decode_hip.hip, under LZH_DEVICE_FUNCTIONS_ONLY, until
the split decoder's device code moves to headers.  zstd_ragged_split_compact_hip.hip needs that device code too, and
the ragged geometry of the split unit; it takes both by including the split unit up to its kernels
(LZH_ZSPLIT_GEOMETRY_ONLY).  That is the same exception, not a second one, as long as what is below holds: the compact
unit is the only file that includes the split unit, only the two of them know the mode, the compact unit does not
reach into decode_hip.hip on its own, and the mode leaves nothing but the split unit's own kernels and launchers out
(the compact unit's kernels stand in a code object of their own).  Reads the sources only."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lzbench_amd", "csrc")
SPLIT_UNIT, COMPACT_UNIT = "zstd_ragged_split_hip.hip", "zstd_ragged_split_compact_hip.hip"


def _sources():
    return {f: open(os.path.join(CSRC, f), encoding="utf-8", errors="replace").read()
            for f in sorted(os.listdir(CSRC)) if f == "Makefile" or f.endswith((".hip", ".h", ".inc", ".cpp", ".c"))}


def test_only_the_compact_unit_includes_the_split_unit():
    assert [f for f, s in _sources().items() if re.search(r'#\s*include\s*"%s"' % re.escape(SPLIT_UNIT), s)] \
        == [COMPACT_UNIT]


def test_the_geometry_mode_is_the_two_units_alone():
    src = _sources()
    assert [f for f, s in src.items() if "LZH_ZSPLIT_GEOMETRY_ONLY" in s] == [COMPACT_UNIT, SPLIT_UNIT]
    assert [f for f, s in src.items() if re.search(r"^\s*#\s*define\s+LZH_ZSPLIT_GEOMETRY_ONLY\b", s, re.M)] \
        == [COMPACT_UNIT]


def test_the_compact_unit_reaches_decode_hip_through_the_split_unit_alone():
    s = _sources()[COMPACT_UNIT]
    assert '#include "decode_hip.hip"' not in s and "LZH_DEVICE_FUNCTIONS_ONLY" not in s
    assert not re.search(r'#\s*include\s*"(?!%s")[^"]*\.hip"' % re.escape(SPLIT_UNIT), s)


def test_the_mode_leaves_out_the_split_units_kernels_and_nothing_before_them():
    """One #ifndef, after the geometry and before the unit's first kernel, closed by the file's last line."""
    s = _sources()[SPLIT_UNIT]
    assert len(re.findall(r"LZH_ZSPLIT_GEOMETRY_ONLY", s)) == 2   # (the #ifndef and the #endif's comment)
    guard = s.index("#ifndef LZH_ZSPLIT_GEOMETRY_ONLY")
    assert "__global__" not in s[:guard] and "hipLaunchKernelGGL" not in s[:guard]
    assert s[guard:].count("__global__") >= 6
    assert s.rstrip().splitlines()[-1].startswith("#endif") and "LZH_ZSPLIT_GEOMETRY_ONLY" in s.rstrip().splitlines()[-1]


def test_the_makefile_builds_the_compact_unit_as_the_split_unit():
    """The pattern rule's flags, the split unit's scheduler setting by reference, and both included files as
    prerequisites of its object."""
    text = re.sub(r"\\\n", " ", _sources()["Makefile"])
    assert re.search(r"^SCHED_zstd_ragged_split_compact\s*=\s*\$\(SCHED_zstd_ragged_split\)\s*$", text, re.M)
    objs = [l for l in text.splitlines() if l.startswith("KOBJ")]
    assert len(objs) == 1 and "/zstd_ragged_split_hip.o" in objs[0] and "/zstd_ragged_split_compact_hip.o" in objs[0]
    dep = [l for l in text.splitlines() if l.startswith("$(OBJDIR)/zstd_ragged_split_compact_hip.o:")]
    assert len(dep) == 1 and set(dep[0].partition(":")[2].split()) == {SPLIT_UNIT, "decode_hip.hip"}
