"""GPU: the zstd entropy kernels on the decisions that tests/test_zstd_entropy_census.py pins -- every named input
(tests/zstd_entropy_inputs.py, the imported edge and level-3 rows included) through the uniform call at each of its
levels and at its row's chunk size against the restatement's bytes (which the CPU test ties to the reference build) and
back through every decoder path of tests/test_gpu_zstd.py's PATHS; the inputs of one block as one ragged batch at
level 1 (plain and compact scratch, in the table's order and permuted: the ragged entropy kernel includes the same
body and reads its frame index, scratch stride and staging slot from other arrays); and all of them through the
level-3 compressor against the reference build's frames (the same literal and sequence shapes at strategy 2's
thresholds; no census claim there).  Every comparison is exact.  Run with -m gpu."""
import numpy as np
import pytest

import lzbench_amd as L
import oracle_lib as O
import zstd_entropy_inputs as I
from gpu_batches import check_batch, place, roundtrip, to_dev, torch_cuda
from test_gpu_zstd import PATHS, expected_sizes, gpu_decode
from test_zstd_entropy_census import row_data, row_packed
from zstd_ragged_inputs import codec_name, expect

pytestmark = pytest.mark.gpu

LEVELS = sorted({lv for r in I.ROWS for lv in r.levels}, reverse=True)
SMALL = [r for r in I.ROWS if len(row_data(r.name)) <= I.BLOCK]
PERMUTATION = np.random.default_rng(5).permutation(len(SMALL)).tolist()


def groups(level):
    """[(chunk size, rows)] of that level: a row with a chunk size is a call of its own, the one-frame rows of one
    size share a call, one chunk each"""
    by, out = {}, []
    for r in I.ROWS:
        if level not in r.levels:
            continue
        if r.chunk:
            out.append((r.chunk, [r]))
        else:
            by.setdefault(max(len(row_data(r.name)), 1), []).append(r)
    return out + sorted(by.items())


@pytest.mark.parametrize("level", LEVELS)
def test_uniform_call(torch_cuda, level):
    for chunk, rows in groups(level):
        data = np.concatenate([row_data(r.name) for r in rows])
        want = [row_packed(r.name, level) for r in rows]
        ep = b"".join(p.tobytes() for p, _ in want)
        ecs = np.concatenate([cs for _, cs in want])
        gp, gcs = L.compress_chunks(data, codec_name(level), chunk, level=level)
        names = [r.name for r in rows]
        assert (np.asarray(gcs) == ecs).all(), (names, level, gcs, ecs)
        assert gp.tobytes() == ep, (names, level)
        for r, (p, cs) in zip(rows, want):                   # the recorded sizes
            if r.chunk or len(p) != len(row_data(r.name)):   # (a one-frame row stored raw has no frame to measure)
                assert len(p) == r.packed[level], r.name
        for path in PATHS:
            st, out = gpu_decode(torch_cuda, gp, gcs, len(data), chunk, path)
            assert (st == expected_sizes(len(data), chunk)).all(), (names, level, path, st)
            assert (out == data).all(), (names, level, path)


@pytest.mark.parametrize("order", ["table", "permuted"])
@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
def test_ragged_batch_level_1(torch_cuda, compact, order):
    torch = torch_cuda
    rows = SMALL if order == "table" else [SMALL[i] for i in PERMUTATION]
    assert all(1 in r.levels for r in rows)
    host, offs, sizes = place([row_data(r.name) for r in rows])
    rc = L.RaggedCodec("zstd", max(sizes), len(sizes), 1, max_total_bytes=sum(sizes), compact_scratch=compact)
    rc.compress(to_dev(torch, host), offs, sizes)
    frames = [expect(row_data(r.name), 1) for r in rows]       # frame i: the uniform call's bytes of input i
    check_batch(torch, rc, len(sizes), frames)
    roundtrip(torch, rc, host, offs, sizes)


def test_level_3_against_the_reference_build(torch_cuda):
    if not O.have_ref():
        pytest.skip("reference build (oracle/_ref) not present: nothing to compare level 3 with")
    by = {}
    for r in I.ROWS:
        by.setdefault((r.chunk or max(len(row_data(r.name)), 1), r.name if r.chunk else ""), []).append(r)
    for (chunk, _), rs in sorted(by.items()):
        data = np.concatenate([row_data(r.name) for r in rs])
        gp, gcs = L.compress_chunks(data, "zstd_dfast", chunk, level=3)
        rp, rcs = O.compress_chunks(data, "zstd", chunk, 3, use_ref=True)
        assert (np.asarray(gcs) == rcs).all(), ([r.name for r in rs], gcs, rcs)
        assert gp.tobytes() == rp.tobytes(), [r.name for r in rs]
