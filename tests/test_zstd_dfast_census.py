"""CPU: the host census of the level-3 (double-fast) walk (tests/zstd_dfast_census.py, oracle/zstd_dfast_census.cpp)
anchored to the reference build, and the named inputs (tests/zstd_dfast_inputs.py) against their declarations.  The
walk is the kernel's own template, so nothing here compares it with itself: for every named input and every case of
tests/zstd_dfast_cases.py
  * its sequences replay to the input byte for byte, every offset inside the window;
  * for every compressed block of the reference build's level-3 frame, its sequence count equals the block's nseq
    and its literal bytes the block's regenerated literal size (tests/zstd_census.py walk()); the repcodes of a block
    the reference stored raw or as RLE are not confirmed, as zstd_compress.c:3813 has it;
  * its sequences equal ZSTD_generateSequences' (literal length, match length, resolved offset, last literals),
    block by block.  That function confirms the repcodes after every block and collects nothing for a block under 7
    bytes (zstd_compress.c:3784-3788, :2821), so the comparison is made only for frames of `block/cmp` blocks alone;
  * no invariant counter moved.
Then: every class of the census is reached by a named input or a fixture case, except the ones listed UNREACHABLE with
their arguments, which no input may reach; the committed digests of the named inputs are the reference build's; and
the frame-format classes (tests/zstd_census.py) of the level-3 frames are pinned.  All of it needs the reference
build (oracle/_ref) and skips without it."""
import json
import os
import sys
from collections import Counter

import pytest

import oracle_lib as O
import zstd_census as ZC
import zstd_dfast_cases as Z
import zstd_dfast_census as D
import zstd_dfast_inputs as I

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
pytestmark = pytest.mark.skipif(not (O.have_ref() and D.have_lib()), reason="reference build (oracle/_ref) not present")

# the fixture cases as frames: a case of several chunks contributes its first and its last chunk
CASE_FRAMES = []
for _name, _kind, _n, _chunk in Z.cases():
    _starts = sorted({0, max((_n - 1) // _chunk, 0) * _chunk})
    CASE_FRAMES += [(f"{_name}@{s}", _kind, _n, s, min(_chunk, _n - s)) for s in _starts]

_cache = {}


def anchored(key, make):
    """(Counter, frame-format Counter, all-cmp) of one frame, every check of the docstring made once"""
    if key in _cache:
        return _cache[key]
    data = make()
    frame = D.ref_frame(data)
    types = D.block_types(frame)
    c, blocks, seqs = D.walk(data, [t == "cmp" for t in types])
    assert len(blocks) == len(types), (key, len(blocks), types)
    assert D.rebuild(data, blocks, seqs) == data.tobytes(), f"{key}: the sequences do not rebuild the input"
    fc, ref_blocks, fcs = ZC.walk(frame)
    assert fcs == len(data)
    mine = [(b[1], b[0]) for b, t in zip(blocks, types) if t == "cmp"]
    assert mine == ref_blocks, f"{key}: (literal bytes, sequences) per compressed block differ from the reference frame"
    assert all(b[3] or (b[0] == 0 and b[1] == b[2] < 7) for b in blocks)
    all_cmp = len(data) > 0 and all(t == "cmp" for t in types)
    if all_cmp and D.have_ref_sequences():
        ref = D.ref_sequences(data)
        assert len(ref) == len(blocks), key
        s = 0
        for k, ((rs, tail), b) in enumerate(zip(ref, blocks)):
            got = [(ll, ml, off) for ll, _, ml, off in seqs[s:s + b[0]].tolist()]
            s += b[0]
            assert got == [(ll, ml, off) for ll, ml, off, _ in rs], f"{key}: block {k} differs from ZSTD_generateSequences"
            assert tail == b[2], (key, k)
    for name in D.INVARIANTS:
        assert not c[name], (key, name, c[name])
    _cache[key] = (c, fc, all_cmp)
    return _cache[key]


def test_class_table_is_the_librarys():
    assert D.classes() == D.documented()
    assert set(D.UNREACHABLE) <= set(D.classes())
    for i in I.INPUTS:
        assert set(i.classes) <= set(D.classes()) - set(D.UNREACHABLE), i.name


@pytest.mark.parametrize("inp", I.INPUTS, ids=lambda i: i.name)
def test_named_input_is_anchored_and_reaches_its_classes(inp):
    c, _, _ = anchored(inp.name, inp.make)
    for cl in inp.classes:
        assert c[cl], f"{inp.name} does not reach {cl}: {dict(c)}"


@pytest.mark.parametrize("case", CASE_FRAMES, ids=lambda c: c[0])
def test_fixture_case_is_anchored(case):
    key, kind, n, start, size = case
    anchored(key, lambda: Z.corpus(kind, n)[start:start + size].copy())


def test_exact_lengths_of_the_built_inputs():
    """the dense inputs have the literal runs and the forward counts they were built for, one each"""
    c = anchored("lits", I.BY_NAME["lits"].make)[0]
    assert c["sequences"] == len(I._LITS) and (c["lit/64"], c["lit/256"], c["lit/>256"]) == (1, 1, 2)
    # (the first run is the head and one byte: 241)
    assert (c["lit/1-63"], c["lit/65-255"]) == (1, 3) and c["step/2"] >= 1
    c = anchored("counts", I.BY_NAME["counts"].make)[0]
    assert c["sequences"] == len(I._COUNTS) and c["search/long-hit"] >= 1
    assert (c["count/1-255"], c["count/256"], c["count/257-511"], c["count/512+"]) == (1, 1, 2, 2)
    for name, cls in (("catchup64", "catchup/64"), ("catchup70", "catchup/65+"), ("lit65536", "lit/>=65536")):
        c = anchored(name, I.BY_NAME[name].make)[0]
        assert c["sequences"] == 1 == c[cls], (name, dict(c))


def test_sequence_comparison_applies_to_most_inputs():
    """the sequence-by-sequence comparison is restricted to all-cmp frames: it must still cover the built inputs"""
    if not D.have_ref_sequences():
        pytest.skip("the reference build lacks ref_zstd_generate_sequences")
    compared = [i.name for i in I.INPUTS if anchored(i.name, i.make)[2]]
    for name in ("counts", "lits", "step3", "step4", "catchup64", "catchup70", "lit65536", "nseq32", "nseq64",
                 "mixed270000", "text140000"):
        assert name in compared, name


def test_every_class_is_reached_or_argued_unreachable():
    named, cases = Counter(), Counter()
    for i in I.INPUTS:
        named.update(anchored(i.name, i.make)[0])
    for case in CASE_FRAMES:
        key, kind, n, start, size = case
        cases.update(anchored(key, lambda: Z.corpus(kind, n)[start:start + size].copy())[0])
    reached = named + cases
    turned_up = [c for c in D.UNREACHABLE if reached[c]]
    assert not turned_up, f"classes argued unreachable turned up: {turned_up}"
    missing = [c for c in D.classes() if not reached[c] and c not in D.UNREACHABLE]
    assert not missing, missing
    # the named inputs alone reach all of them as well; the fixture cases are not needed for any class
    assert not [c for c in D.classes() if not named[c] and c not in D.UNREACHABLE]
    small = Counter()
    for i in I.INPUTS:
        if i.name != I.FAR:
            small.update(anchored(i.name, i.make)[0])
    only_far = sorted(c for c in D.classes() if named[c] and not small[c])
    print("\nclasses only the multi-megabyte input reaches:", only_far)
    assert only_far == sorted(ONLY_FAR)
    print("classes the fixture cases do not reach:", sorted(c for c in D.classes() if named[c] and not cases[c]))


# the window slides only in a frame over 2 MiB (below that the window log is the source's)
ONLY_FAR = {"block/dl>0", "block/plow>dl", "reject/long/stale", "reject/short/stale"}


def test_committed_digests_are_the_reference_builds():
    import make_zstd_dfast_census_golden as M
    with open(os.path.join(GOLD, "zstd_dfast_census_golden.json")) as f:
        g = json.load(f)
    assert g["version"] == int(O.ref().ref_zstd_version())
    assert [c["name"] for c in g["cases"]] == [i.name for i in I.INPUTS]
    for c, i in zip(g["cases"], I.INPUTS):
        assert M.entry(i) == c, i.name


FORMAT_DID_NOT_OCCUR = {"lit/regen=0", "lit/rle/hdr1", "lit/rle/hdr2", "lit/rle/hdr3", "lit/treeless/sf0",
                        "lit/treeless/sf3", "nseq/long"}


# frame-format classes (tests/zstd_census.py) the level-3 frames of the named inputs and the fixture cases do not take.
# {LL,OF,ML}/repeat cannot occur at level 3 without a dictionary: below ZSTD_lazy, ZSTD_selectEncodingType
# (zstd_compress_sequences.c:179-204) returns set_repeat only for FSE_repeat_valid, which only a dictionary's tables
# carry (a compressed block leaves FSE_repeat_check, :206 on).  The rest (FORMAT_DID_NOT_OCCUR) is possible but did not occur
# in these frames: RLE literals and a block without literals need a block whose literals are one repeated byte or none
# (level 1 has them: tests/test_zstd_census.py), treeless sections came in the 10- and 14-bit size formats only,
# nseq/long needs 32512 sequences in one block.
FORMAT_NOT_REACHED = {"LL/repeat", "OF/repeat", "ML/repeat"} | FORMAT_DID_NOT_OCCUR


def test_frame_format_census_of_level3():
    fc = Counter()
    for i in I.INPUTS:
        fc.update(anchored(i.name, i.make)[1])
    for case in CASE_FRAMES:
        key, kind, n, start, size = case
        fc.update(anchored(key, lambda: Z.corpus(kind, n)[start:start + size].copy())[1])
    must = ([f"{t}/{m}" for t in ("LL", "OF", "ML") for m in ("predef", "rle", "fse")]
            + ["hufhdr/fse", "hufhdr/direct", "block/raw", "block/rle", "block/cmp", "nseq/0"])
    assert not [c for c in must if not fc[c]], [c for c in must if not fc[c]]
    assert any(fc[f"lit/treeless/sf{s}"] for s in range(4))
    not_reached = {c for c in ZC.ALL_CLASSES if not fc[c]}
    print("\nframe-format classes the level-3 frames do not take:", sorted(not_reached))
    assert not_reached == FORMAT_NOT_REACHED
