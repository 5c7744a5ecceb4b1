"""GPU: the zstd kernels on the branches of the frame format that tests/test_zstd_census.py pins -- the named edge
inputs (tests/zstd_edge_inputs.py) through the uniform and the ragged compressor against the restatement and the
reference build byte for byte, their frames and the repeat-mode fixture (tests/golden/make_zstd_repeat.py)
through the four decoder paths and the ragged decoders, and the hand-built frames no encoder writes
(tests/zstd_hand_frames.py) with the reference's verdict and bytes.  Every comparison is exact.  The census union
of what ran is printed once.  Run with -m gpu.

Found by these inputs: `tail_repeat` (a 61072-byte match at offset 70000) and `rle_literals` (a 131072-byte match at
offset 131072) decoded wrong on every path -- a match whose source is out of the LDS output window and that does
not overlap itself was written through the window without a flush, so one longer than the window wrapped it
(owin::SinkT::match, lzbench_amd/csrc/decode_win.h).  Both stay here as its tests."""
from collections import Counter

import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
import zstd_census as Z
import zstd_edge_inputs as E
import zstd_hand_frames as H
from test_gpu_zstd import PATHS, expected_sizes, gpu_decode
from gpu_batches import check_batch, layout, roundtrip, to_dev, torch_cuda
from zstd_ragged_inputs import codec_name, expected
from test_gpu_zstd_ragged_split import decode_frames
from test_zstd_census import (EDGE_ROWS, edge_data, edge_packed, ref_decode, repeat_arrays, repeat_cases,
                              repeat_corpus)

pytestmark = pytest.mark.gpu

_ran = Counter()          # the census of every frame a test here compressed to or decoded


def _edge(name):
    return next(e for e in E.EDGES if e.name == name)


def _frames(packed, cs, data, chunk):
    """[(frame or raw-stored bytes, chunk bytes)] of a packed stream"""
    out, pos = [], 0
    for i, s in enumerate(cs):
        out.append((np.asarray(packed[pos: pos + int(s)]).tobytes(), data[i * chunk: (i + 1) * chunk]))
        pos += int(s)
    return out


# ---- a. the uniform compressor ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", EDGE_ROWS, ids=[f"{n}-l{lv}" for n, lv in EDGE_ROWS])
def test_uniform_compress_rows(torch_cuda, name, level):
    e, data = _edge(name), edge_data(name)
    ep, ecs = edge_packed(name, level)
    gp, gcs = L.compress_chunks(data, codec_name(level), e.chunk, level=level)
    assert (gcs == ecs).all(), (gcs, ecs)
    assert len(gp) == len(ep) == e.packed[level] and gp.tobytes() == ep.tobytes(), "GPU and restatement differ"
    if O.have_ref():
        rp, rcs = O.compress_chunks(data, "zstd", e.chunk, level, use_ref=True)
        assert (gcs == rcs).all() and gp.tobytes() == rp.tobytes(), "GPU and reference build differ"
    out = L.decompress_chunks(gp, gcs, len(data), "zstd", e.chunk)
    assert (out == data).all()
    _ran.update(Z.census_packed(gp, gcs, len(data), e.chunk)[0])


# ---- b. the decoder paths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,level", EDGE_ROWS, ids=[f"{n}-l{lv}" for n, lv in EDGE_ROWS])
def test_decoder_paths_on_edge_frames(torch_cuda, name, level, path):
    e, data = _edge(name), edge_data(name)
    packed, cs = edge_packed(name, level)
    st, out = gpu_decode(torch_cuda, packed, cs, len(data), e.chunk, path)
    assert (st == expected_sizes(len(data), e.chunk)).all(), st
    assert (out == data).all()
    _ran.update(Z.census_packed(packed, cs, len(data), e.chunk)[0])


# ---- c. the ragged compressor and decoders ------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, -5, 2])
def test_ragged_batch_of_single_block_inputs(torch_cuda, level):
    torch = torch_cuda
    edges = E.single_block_edges(level)
    assert edges and all(len(edge_data(e.name)) <= E.BLOCK for e in edges)      # (level 2: nothing above 128 KiB)
    parts = [edge_data(e.name) for e in edges]
    parts += [p[:n] for p in parts for n in (len(p) - 1, 65543)]     # each input once more cut shorter
    sizes = [len(p) for p in parts]
    offs, total = layout(sizes)
    host = np.zeros(total, np.uint8)
    for o, p in zip(offs, parts):
        host[o: o + len(p)] = p
    for split in (True, False):
        rc = L.RaggedCodec(codec_name(level), max(sizes), len(sizes), level, max_total_bytes=sum(sizes),
                           split_decode=split)
        rc.compress(to_dev(torch, host), offs, sizes)
        cs, of, packed = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level))
        roundtrip(torch, rc, host, offs, sizes)
    for i, e in enumerate(edges):        # the whole inputs' frames are the uniform call's for a chunk of that size
        assert int(cs[i]) == e.packed[level]
        _ran.update(Z.census(packed[of[i]: of[i + 1]].tobytes()))


def _decode_everywhere(torch, frames, contents):
    """frames through the four paths of the uniform call, one frame a call, and as one ragged batch through the
    split decoder and the one-wave decoder: every status is the content size, every byte the content's"""
    for path in PATHS:
        for f, want in zip(frames, contents):
            n = len(want)
            st, out = gpu_decode(torch, np.frombuffer(f, np.uint8), [len(f)], n, max(n, E.BLOCK), path)
            assert st.tolist() == [n], (path, st)
            assert out.tobytes() == bytes(want), path
    sizes = [len(c) for c in contents]
    for split in (True, False):
        st, got, offs = decode_frames(torch, frames, sizes, max(max(sizes), 16384), split)[:3]
        mask = np.zeros(len(got), bool)
        for i, want in enumerate(contents):
            assert int(st[i]) == len(want), (split, i, st)
            assert got[offs[i]: offs[i] + len(want)].tobytes() == bytes(want), (split, i)
            mask[offs[i]: offs[i] + len(want)] = True
        assert (got[~mask] == 0xEE).all(), "write outside the chunks"
    for f in frames:
        _ran.update(Z.census(f))


# ---- d. frames no encoder writes ----------------------------------------------------------------------------------
def test_hand_built_frames(torch_cuda):
    frames, contents = [], []
    for name, f, content in H.hand_frames():
        if O.have_ref():                 # the reference's verdict and bytes come first
            r, out = ref_decode(f, len(content))
            assert r == len(content), f"the reference rejects {name}: the frame is wrong"
            assert out == content
        frames.append(f)
        contents.append(content)
    _decode_everywhere(torch_cuda, frames, contents)


# ---- e. table modes only higher levels write ----------------------------------------------------------------------
def test_repeat_mode_fixture(torch_cuda):
    A = repeat_arrays()
    frames, contents = [], []
    for c in repeat_cases():
        data = repeat_corpus(c)
        for f, part in _frames(A[c["name"] + "/packed"], A[c["name"] + "/csizes"], data, c["chunk"]):
            assert len(f) != len(part)
            frames.append(f)
            contents.append(part.tobytes())
    u = sum((Z.census(f) for f in frames), Counter())
    assert u["LL/repeat"] and u["OF/repeat"] and u["ML/repeat"]
    _decode_everywhere(torch_cuda, frames, contents)


def test_zz_print_census():
    """(last in the file) the classes the tests above ran, and the ones they did not"""
    print("\nzstd census of this file's GPU runs:", dict(sorted(_ran.items())))
    print("not run here:", sorted(set(Z.ALL_CLASSES) - set(k for k in _ran if _ran[k])))
