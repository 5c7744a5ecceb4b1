"""CPU: the census of the zstd entropy stage's decisions (tests/zstd_entropy_census.py, oracle_zstd_compress_census) and
the named inputs that reach them (tests/zstd_entropy_inputs.py): the counting call writes oracle_zstd_compress's
bytes, those are the reference build's (oracle/_ref, where present), every row has its recorded size and its declared
classes, every class is documented, and every class is reached by a named input, argued unreachable and absent, or
listed as not reached.  The GPU runs the same rows in tests/test_gpu_zstd_entropy_census.py."""
import functools
from collections import Counter

import numpy as np
import pytest

import oracle_lib as O
import zstd_edge_inputs as E
import zstd_entropy_census as ZE
import zstd_entropy_inputs as I
from test_zstd_oracle import cgolden, corpus as ccorpus

ROW_LEVELS = [(r.name, lv) for r in I.ROWS for lv in r.levels]


@functools.lru_cache(maxsize=None)
def row_data(name):
    d = np.ascontiguousarray(next(r for r in I.ROWS if r.name == name).make())
    d.setflags(write=False)
    return d


def row_of(name):
    return next(r for r in I.ROWS if r.name == name)


@functools.lru_cache(maxsize=None)
def row_packed(name, level):
    """what the GPU must write for a row at one of its levels, from the restatement: (packed bytes, csizes) with the
    raw-store rule of lzbench's loop, at the row's chunk size (a row of one frame: its own size)"""
    data = row_data(name)
    return O.compress_chunks(data, "zstd", row_of(name).chunk or max(len(data), 1), level, use_ref=False)


@functools.lru_cache(maxsize=None)
def row_census(name, level):
    row = row_of(name)
    return ZE.walk_chunks(row_data(name), row.chunk, level) if row.chunk else ZE.walk(row_data(name), level)[1]


def ref_frame(data, level):
    dst = np.zeros(len(data) + len(data) // 128 + 1024, np.uint8)
    r = O.ref().ref_zstd_compress(data.ctypes.data, len(data), dst.ctypes.data, len(dst), level)
    assert r > 0
    return dst[:r].tobytes()


@pytest.mark.parametrize("name,level", ROW_LEVELS, ids=[f"{n}-l{lv}" for n, lv in ROW_LEVELS])
def test_row_bytes_size_and_classes(name, level):
    row = row_of(name)
    data = row_data(name)
    c = row_census(name, level)
    if row.chunk:                        # a row of lzbench's loop: the packed stream
        packed, cs = row_packed(name, level)
        assert len(packed) == row.packed[level]
        if O.have_ref():                 # (without the reference build only this comparison is left out)
            rp, rcs = O.compress_chunks(data, "zstd", row.chunk, level, use_ref=True)
            assert (rcs == cs).all() and rp.tobytes() == packed.tobytes(), "restatement and reference build differ"
    else:
        frame = ZE.walk(data, level)[0]
        assert frame == O.zstd_compress(data, level), "the counting call writes other bytes"
        if O.have_ref():
            assert frame == ref_frame(data, level), "restatement and reference build differ"
        assert len(frame) == row.packed[level]
    want = dict(row.classes if level == 1 else {}, **row.at.get(level, {}))
    assert want or level != 1, "a row declares what it is there for"
    short = {k: (c[k], v) for k, v in want.items() if c[k] < v}
    assert not short, f"classes lost (have, want): {short}"
    assert not any(c[k] for k in ZE.UNREACHABLE), {k: c[k] for k in ZE.UNREACHABLE if c[k]}


def test_counting_call_writes_the_same_bytes_chunk_by_chunk():
    """the rows of lzbench's loop: every chunk's frame from the counting call is oracle_zstd_compress's"""
    for row in I.ROWS:
        if row.chunk:
            data = row_data(row.name)
            for lv in row.levels:
                for a in range(0, len(data), row.chunk):
                    part = np.ascontiguousarray(data[a: a + row.chunk])
                    assert ZE.walk(part, lv)[0] == O.zstd_compress(part, lv), (row.name, lv, a)


def test_rows_are_small():
    sizes = [len(row_data(r.name)) for r in I.ROWS]
    assert len(I.ROWS) <= 40 and sum(sizes) <= 6 << 20
    # (the rows built here; an imported row has the size its own file gives it)
    assert all(len(row_data(r.name)) <= 3 * I.BLOCK for r in I.ROWS if ":" not in r.name)


def test_every_class_is_documented():
    """DOC (class -> reference line, kernel branch) names exactly the classes of the list, each with both parts, and
    the module's docstring is rendered from it and from the two sets"""
    assert sorted(ZE.documented()) == sorted(ZE.ALL_CLASSES)
    assert all(len(v) == 2 and all(v) for v in ZE.DOC.values())
    for k in list(ZE.DOC) + list(ZE.UNREACHABLE) + list(ZE.NOT_REACHED):
        assert f"\n  {k}   " in ZE.__doc__, k
    assert all(len(v) > 8 for v in list(ZE.UNREACHABLE.values()) + list(ZE.NOT_REACHED.values()))


def declared():
    d = set()
    for r in I.ROWS:
        d.update(r.classes)
        for m in r.at.values():
            d.update(m)
    return d


def test_three_sets_cover_the_class_list():
    reached, un, nr = declared(), set(ZE.UNREACHABLE), set(ZE.NOT_REACHED)
    assert reached | un | nr == set(ZE.ALL_CLASSES), sorted(set(ZE.ALL_CLASSES) - reached - un - nr)
    assert not reached & un and not reached & nr and not un & nr


MUST_BE_REACHED = (
    ["lit/gate/n=63", "lit/gate/n=64", "lit/sampled/raw", "lit/flat/raw", "lit/rle", "lit/repeat/invalid",
     "lit/repeat/small-direct", "lit/repeat/new-table", "lit/hdr/3", "lit/hdr/4", "lit/hdr/5", "lit/streams/1",
     "lit/streams/4", "huf/limit/fired", "huf/limit/not-needed", "huf/table/direct", "huf/table/fse",
     "seq/ns/1", "seq/ns/64", "seq/ns/65", "block/rle", "block/raw/mingain", "block/repcodes-unconfirmed"]
    + [f"seq/ns%64/{r}" for r in range(6)])
MUST_BE_REACHED_ANY = (        # one of each group
    ("lit/repeat/old-by-estimate", "lit/repeat/old-by-h+12"),
    ("seqtab/norm/fast", "hufw/norm/fast"), ("seqtab/norm/low/-1",), ("seqtab/norm/low/+1", "hufw/norm/low/+1"),
    ("seqtab/ncount/zero-run/3+", "hufw/ncount/zero-run/3+"),
    tuple(f"seq/{t}/type/rle" for t in ZE.TABLES), tuple(f"seq/{t}/type/rle-as-predef" for t in ZE.TABLES),
    tuple(f"seq/{t}/type/predef-by-count" for t in ZE.TABLES), tuple(f"seq/{t}/type/fse" for t in ZE.TABLES),
    tuple(f"seq/{t}/last-count-trick/taken" for t in ZE.TABLES),
    tuple(f"seq/{t}/last-count-trick/not" for t in ZE.TABLES))


def test_not_reached_holds_none_of_the_required():
    reached = declared()
    assert not set(MUST_BE_REACHED) - reached
    assert all(any(k in reached for k in group) for group in MUST_BE_REACHED_ANY)
    assert "seq/OF/type/default-refused" in ZE.UNREACHABLE


def test_not_reached_is_short():
    """the issue allows six"""
    assert len(ZE.NOT_REACHED) <= 6, ZE.NOT_REACHED


# the classes the corpora of tests/test_zstd_oracle.py (the committed digests' cases) and the rows of
# tests/zstd_edge_inputs.py do not reach: the ones a named input of tests/zstd_entropy_inputs.py carries alone
ONLY_NAMED = {
    "lit/gate/n=63", "lit/suspect/ratio=19", "lit/suspect/ratio=20", "lit/raw/streams-too-large/old",
    "lit/raw/streams-too-large/new", "lit/raw/mingain", "huf/weights/wn<=1", "huf/weights/all-distinct",
    "seq/ns%64/5", "seq/ns/64", "seq/ns/65", "seq/ns/128", "seq/ns/129", "seq/bits/>=57", "hufw/ncount/zero-run/3+",
    "seq/LL/last-count-trick/not", "norm/m2/second-pass", "seq/ML/type/predef-by-flatness"}


@functools.lru_cache(maxsize=None)
def corpora_census():
    u = Counter()
    for c in cgolden():
        u.update(ZE.walk_chunks(ccorpus(c["corpus"], c["n"], c["seed"]), c["chunk"], c["level"]))
    for e in E.EDGES:
        d = e.make()
        for lv in e.levels:
            u.update(ZE.walk_chunks(d, e.chunk, lv))
    return u


def test_what_the_existing_corpora_reach():
    u = corpora_census()
    assert not any(u[k] for k in ZE.UNREACHABLE), {k: u[k] for k in ZE.UNREACHABLE if u[k]}
    assert not any(u[k] for k in ZE.NOT_REACHED), {k: u[k] for k in ZE.NOT_REACHED if u[k]}
    missing = {k for k in ZE.ALL_CLASSES if not u[k]} - set(ZE.UNREACHABLE) - set(ZE.NOT_REACHED)
    table = "\n".join(f"{k:44s} {u[k]}" for k in ZE.ALL_CLASSES)
    assert missing == ONLY_NAMED, f"only named inputs reach {sorted(missing)}\n{table}"
