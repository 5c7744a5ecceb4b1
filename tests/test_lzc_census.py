"""CPU: the named compressor inputs (tests/lzc_inputs.py) against their declarations -- every row compresses in the
restatement to its pinned size, to the reference build's bytes where that build is present, reaches the parser
events (tests/lzc_census.py) it claims, and the rows together reach every class the census names.  The last test
lists what the synthetic corpora reach by themselves, so the classes only the named inputs cover are on record."""
from collections import Counter

import numpy as np
import pytest

import lzbench_amd as L
import lzc_census as Z
import lzc_inputs as I
import oracle_lib as O

ROWS = I.rows()
IDS = [f"{i.name}-l{lv}" for i, lv in ROWS]
_data, _cens = {}, {}


def data_of(inp):
    if inp.name not in _data:
        d = inp.make()
        _data[inp.name] = d
    return _data[inp.name]


def census_of(inp, level):
    """(compressed bytes, Counter) of a row, computed once"""
    key = (inp.name, level)
    if key not in _cens:
        _cens[key] = Z.census(I.codec_of(inp, level), data_of(inp), level)
    return _cens[key]


def ref_bytes(inp, level):
    d = np.ascontiguousarray(data_of(inp))
    dst = np.zeros(len(d) + len(d) // 6 + 1024, np.uint8)
    R = O.ref()
    if inp.codec == "snappy":
        r = R.ref_snappy_compress(d.ctypes.data, len(d), dst.ctypes.data)
    else:
        r = R.ref_lz4_compress_fast(d.ctypes.data, dst.ctypes.data, len(d), len(dst), level)
    return dst[:r].tobytes()


def test_names_are_unique_and_declared_classes_exist():
    assert len({i.name for i in I.INPUTS}) == len(I.INPUTS)
    for i in I.INPUTS:
        for c in tuple(i.classes) + tuple(c for cs in i.classes_at.values() for c in cs):
            assert f"{i.codec}/{c}" in Z.ALL_CLASSES, (i.name, c)
        assert set(i.packed) == set(i.levels), i.name


@pytest.mark.parametrize("inp,level", ROWS, ids=IDS)
def test_row_size_bytes_and_classes(inp, level):
    d = data_of(inp)
    out, c = census_of(inp, level)
    assert len(out) == inp.packed[level]
    # the counting entry point writes what the plain one writes
    plain = O.snappy_compress(d) if inp.codec == "snappy" else O.lz4_compress(d, level)
    assert out == plain
    if O.have_ref():
        assert out == ref_bytes(inp, level), "restatement and reference build differ"
    for cl in tuple(inp.classes) + tuple(inp.classes_at.get(level, ())):
        assert c[f"{inp.codec}/{cl}"], f"{inp.name} at level {level} does not reach {cl}: {dict(c)}"
    if inp.codec == "lz4":
        assert c["lz4/sequences"] == c["lz4/hit/search"] + c["lz4/hit/retest"]


def test_exact_literal_runs_and_matches():
    """the spliced inputs have the literal runs and the match lengths they were built for, one each"""
    _, c = census_of(next(i for i in I.INPUTS if i.name == "lits"), 1)
    # _LITS: 14 | 15 | 16, 255 | 256, 257, 269, 270, 271 (and the first sequence's literals: the head)
    assert (c["lz4/lit/1-14"], c["lz4/lit/15"], c["lz4/lit/16-255"], c["lz4/lit/256+"], c["lz4/lit/270"]) == (1, 1, 3, 5, 1)
    _, c = census_of(next(i for i in I.INPUTS if i.name == "matches"), 1)
    # _MATCHES - 4: 14, 15, 16, 19 | 20 | 21, 269, 270, 271, 275 | 276 (and the first sequence: 8 - 4)
    assert (c["lz4/count/1-19"], c["lz4/count/20"], c["lz4/count/21-275"], c["lz4/count/>275"]) == (5, 1, 5, 1)
    assert c["lz4/ml/15"] == 1 and c["lz4/ml/15+255"] == 1
    for k in (0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 300):
        inp = next(i for i in I.INPUTS if i.name == f"catchup{k}")
        _, c = census_of(inp, inp.levels[0])
        assert c["lz4/hit/search"] == 1 == sum(v for n, v in c.items() if n.startswith("lz4/catchup/")), inp.name


def _tags(name):
    return Z.snappy_tags(census_of(next(i for i in I.INPUTS if i.name == name), 0)[0])


def test_exact_snappy_literals_and_copies():
    """the snappy inputs built for one literal run or one copy have exactly that one, read back from the stream.  The
    literal lengths are the ends of the three length forms (60 | 61, 256 | 257, 65536).  Before a copy a literal can
    only end at a probe of its search (lzc_inputs.sn_literal): 61, and 254 / 262 around 256; the others end a
    fragment."""
    for lit in (60, 61, 256, 257):
        assert _tags(f"lit{lit}") == [("lit", 21), ("copy", 59, 1), ("lit", lit)]
    for lit, m in ((61, 30), (254, 30), (262, 31)):
        t = _tags(f"lit{lit}copy")
        assert t[2] == ("lit", lit) and t[3][:2] == ("copy", m) and t[4] == ("lit", 41) and len(t) == 5, t
    assert _tags("literal65536")[0] == ("lit", 65536) and _tags("random65536") == [("lit", 65536)]
    for off in (2047, 2048):
        for m in (11, 12, 64, 65, 67, 68, 131, 132):
            t = _tags(f"copy{m}at{off}")
            i = next(k for k, x in enumerate(t) if x[0] == "copy" and x[2] == off)
            j = i
            while j < len(t) and t[j][0] == "copy" and t[j][2] == off:
                j += 1
            assert sum(x[1] for x in t[i:j]) == m and t[i - 1] == ("lit", 7) and t[j][0] == "lit", (m, off, t)
            # EmitCopy's pieces: 64s while 68 or more are left, 60 when 65..67 are, then the rest
            want = [64] * max((m - 4) // 64, 0)
            rest = m - sum(want)
            want += [60, rest - 60] if rest > 64 else [rest]
            assert [x[1] for x in t[i:j]] == want, (m, off, t[i:j])


def test_union_covers_every_class():
    u = Counter()
    for inp, level in ROWS:
        u.update(census_of(inp, level)[1])
    assert not [c for c in Z.ALL_CLASSES if not u[c]]


def test_zz_what_the_corpora_reach():
    """(printed) the classes one 1 MiB sample of each datagen kind reaches at chunks of 64 and 256 KiB, and the ones
    only the named inputs reach; the latter are pinned so that a corpus change that starts to cover one shows"""
    u = Counter()
    for kind in ("random", "text", "json", "mixed", "binary"):
        d = L.datagen(kind, 1 << 20, seed=12345)
        for chunk in (65536, 262144):
            for at in range(0, len(d), chunk):
                for codec in ("lz4", "snappy"):
                    u.update(Z.census(codec, d[at: at + chunk])[1])
    only = [c for c in Z.ALL_CLASSES if not u[c]]
    print("\nclasses the corpora reach:", sorted(c for c in Z.ALL_CLASSES if u[c]))
    print("classes only tests/lzc_inputs.py reaches:", only)
    assert set(only) >= ONLY_INPUTS, sorted(ONLY_INPUTS - set(only))


# classes no corpus sample above reaches (acceleration 1; a subset is asserted: a richer corpus may reach more)
ONLY_INPUTS = {"lz4/n<13", "lz4/count/>262164", "lz4/far/65536", "lz4/off/65535", "lz4/step>acc", "snappy/frag<15"}
