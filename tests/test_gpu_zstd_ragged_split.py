"""GPU: ragged zstd batches through the four-kernel split decoder (include/lzbench_hip.h 3c,
lzbench_amd.RaggedCodec("zstd", ..., split_decode=True)): with the split temp the statuses and bytes are those of
the one-wave decoder (the small temp), nothing outside the chunks or past the sizing answer is written, and the
frame states in temp (lzh_debug_zstd_ragged_split_layout) tell which decoder finished each frame.
Run with -m gpu."""
import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
from test_zstd_golden import arrays, cases, corpus
import gpu_batches as B
from gpu_batches import check_batch, layout, roundtrip, to_dev, torch_cuda
from zstd_ragged_inputs import codec_name, corpus_mix, expect, expected

pytestmark = pytest.mark.gpu

SPLIT, LEGACY = 2, 1                              # frame states: finished by the split kernels / handed to the one-wave kernel
GUARD = 4096
EDGE_SIZES = [0, 1, 13, 4099, 16384, 65536, 70000, 131072, 131073, 300000]


def region(maxb, k, i):
    """(offset, size) of region i of the split temp (0 offsets, 1 frame areas, 3 frame states); [14] a frame area"""
    v = np.zeros(16, np.uint64)
    assert L.lib().lzh_debug_zstd_ragged_split_layout(maxb, k, v.ctypes.data) == 0
    return int(v[2 * i]), int(v[2 * i + 1]), int(v[14])


def guarded_temp(torch, rc, nbytes):
    """rc.dtemp = exactly nbytes of a 0xEE-filled buffer with GUARD more bytes after it; returns the whole buffer"""
    buf = torch.full((nbytes + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.dtemp = buf[:nbytes]
    return buf


def frame_states(rc, maxb, k):
    off, size, _ = region(maxb, k, 3)
    assert size == 4 * k
    return rc.dtemp[off: off + size].cpu().numpy().view(np.int32)


def split_bytes(maxb, k):
    return L.lib().lzh_zstd_ragged_decompress_split_temp_bytes(maxb, k)


def small_bytes(maxb, k):
    return L.lib().lzh_zstd_ragged_decompress_temp_bytes(maxb, k)


# ---- 1. edge sizes in one batch, every hook ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_input():
    offs, total = layout(EDGE_SIZES)
    host = corpus_mix(total, 23)
    i = EDGE_SIZES.index(131072)                   # a text chunk: four Huffman streams of over 4096 symbols (hufpar)
    host[offs[i]: offs[i] + 131072] = L.datagen("text", 131072, seed=9)
    return host, offs


@pytest.mark.parametrize("level", [1, -5])
def test_edge_sizes_in_one_batch(torch_cuda, edge_input, level):
    torch = torch_cuda
    host, offs = edge_input
    sizes, k, maxb = EDGE_SIZES, len(EDGE_SIZES), 300000
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    rc = L.RaggedCodec(codec_name(level), maxb, k, level, max_total_bytes=sum(sizes), split_decode=True)
    zt, dt = split_bytes(maxb, k), small_bytes(maxb, k)
    assert rc.dtemp.numel() == zt > dt > 0
    rc.compress(to_dev(torch, host), offs, sizes)
    check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level))   # (the restatement's / the reference's frames)
    lib = L.lib()
    big = [i for i, s in enumerate(sizes) if s >= 16384]
    assert len(big) == 6                           # (every frame of 16 KiB and more must end in the split kernels)
    hooks = {"default": None, "huf8": (lib.lzh_debug_zstd_huf_sections, 8, 0), "nopar": (lib.lzh_debug_zstd_hufpar, 0, 1),
             "legacy": (lib.lzh_debug_zstd_legacy, 1, 0)}
    for name, hook in hooks.items():
        buf = guarded_temp(torch, rc, zt)
        try:
            if hook:
                assert hook[0](hook[1]) == 0
            roundtrip(torch, rc, host, offs, sizes)
        finally:
            if hook:
                hook[0](hook[2])
        assert bool((buf[zt:] == 0xEE).all()), f"{name}: write past the split temp"
        st = frame_states(rc, maxb, k)
        if name == "legacy":
            assert (st.view(np.uint32) == 0xEEEEEEEE).all(), "legacy hook: the split kernels ran"
        else:
            print(name, level, "frame states", st.tolist())
            assert all(int(st[i]) == SPLIT for i in big), (name, st.tolist())
            assert set(st.tolist()) <= {SPLIT, LEGACY}
    # the small temp: every frame in the one-wave kernel
    buf = guarded_temp(torch, rc, dt)
    roundtrip(torch, rc, host, offs, sizes)
    assert bool((buf[dt:] == 0xEE).all()), "write past the small temp"
    # a temp one byte short of the split answer decodes one-wave too
    buf = guarded_temp(torch, rc, zt - 1)
    roundtrip(torch, rc, host, offs, sizes)
    off, size, _ = region(maxb, k, 3)
    assert bool((buf[off: off + size] == 0xEE).all()), "temp below the sizing answer: the split kernels ran"


# ---- 2. the boundary of the split decoder ------------------------------------------------------------------------
def test_boundary_chunk_sizes(torch_cuda):
    torch = torch_cuda
    for maxb, sizes in ((16384, [16384, 5000, 16384, 100]), (16383, [16383, 5000, 16383, 100])):
        k = len(sizes)
        offs, total = layout(sizes)
        host = corpus_mix(total, 37)
        rc = L.RaggedCodec("zstd", maxb, k, 1, max_total_bytes=sum(sizes), split_decode=True)
        rc.compress(to_dev(torch, host), offs, sizes)
        check_batch(torch, rc, len(sizes), expected(host, offs, sizes, 1))
        if maxb == 16384:
            assert rc.dtemp.numel() == split_bytes(maxb, k) > 0
            guarded_temp(torch, rc, rc.dtemp.numel())
            roundtrip(torch, rc, host, offs, sizes)
            assert frame_states(rc, maxb, k).tolist() == [SPLIT] * k
        else:                                      # no split decoder below 16 KiB: the small temp, one wave a frame
            assert split_bytes(maxb, k) == 0 and rc.dtemp.numel() == small_bytes(maxb, k)
            roundtrip(torch, rc, host, offs, sizes)


# ---- 3, 4, 6: frames from elsewhere ---------------------------------------------------------------------------------
def decode_frames(torch, frames, out_sizes, maxb, split):
    """frames (bytes each) as one ragged batch with the split or the small temp (d_offsets = NULL):
    (status, output canvas, output offsets, frame states or None)"""
    k = len(frames)
    rc = L.RaggedCodec("zstd", maxb, k, 1, max_total_bytes=sum(out_sizes), split_decode=split)
    nbytes = split_bytes(maxb, k) if split else small_bytes(maxb, k)
    assert nbytes > 0 and rc.dtemp.numel() == nbytes
    buf = guarded_temp(torch, rc, nbytes)
    st, got, offs = B.decode_frames(torch, rc, frames, out_sizes)
    assert bool((buf[nbytes:] == 0xEE).all()), "write past the temp"
    return st, got, offs, frame_states(rc, maxb, k) if split else None


def test_reference_frames(torch_cuda):
    torch = torch_cuda
    A = arrays()
    frames, parts = [], []
    for c in cases():                            # (these include level 3 and level 19 frames, raw and RLE blocks)
        data, packed, cs = corpus(c), A[c["name"] + "/packed"], A[c["name"] + "/csizes"]
        pos = 0
        for i, s in enumerate(cs):
            frames.append(packed[pos: pos + int(s)].tobytes())
            parts.append(data[i * c["chunk"]: (i + 1) * c["chunk"]])
            pos += int(s)
    if O.have_ref():                             # a frame with the content checksum
        part = L.datagen("text", 50_001, seed=6)
        dst = np.zeros(len(part) + 1024, np.uint8)
        r = O.ref().ref_zstd_compress_checksum(part.ctypes.data, len(part), dst.ctypes.data, len(dst), 1)
        assert r > 0
        frames.append(dst[:r].tobytes())
        parts.append(part)
    sizes = [len(p) for p in parts]
    st, got, offs, states = decode_frames(torch, frames, sizes, max(sizes), True)
    mask = np.zeros(len(got), bool)
    for i, p in enumerate(parts):
        assert int(st[i]) == len(p), f"frame {i}: status {st[i]}"
        assert (got[offs[i]: offs[i] + len(p)] == p).all(), f"frame {i}: bytes differ"
        mask[offs[i]: offs[i] + len(p)] = True
    assert (got[~mask] == 0xEE).all()
    print("reference frames: states", states.tolist())
    assert set(states.tolist()) <= {SPLIT, LEGACY}
    assert (states == SPLIT).any()
    # (the golden set alone yields no frame that the split kernels hand to the one-wave kernel -- measured: every
    # state is 2, the level-19 frame included -- so only the range of the states is asserted)


def test_raw_stored_chunk_is_copied(torch_cuda):
    torch = torch_cuda
    raw = L.datagen("random", 4099, seed=2)      # csize == out_bytes: a copy, whatever the bytes are
    text = L.datagen("text", 20000, seed=4)
    st, got, offs, states = decode_frames(torch, [raw.tobytes(), expect(text, 1), raw[:7].tobytes()], [4099, 20000, 7],
                                          20000, True)
    assert st.tolist() == [4099, 20000, 7]
    assert (got[offs[0]: offs[0] + 4099] == raw).all() and (got[offs[1]: offs[1] + 20000] == text).all()
    assert (got[offs[2]: offs[2] + 7] == raw[:7]).all()
    assert states.tolist() == [SPLIT] * 3       # (the header kernel copies a raw-stored chunk)


def test_malformed_frames_get_the_one_wave_verdicts(torch_cuda):
    """The 200 seeded mutations and truncations of test_gpu_zstd_ragged's malformed-frame test (same seed and bases),
    decoded with the split temp and with the small temp: the statuses are equal frame for frame and so are the bytes
    of every chunk that decoded; a rejected chunk may hold different partial output inside the chunk (the split
    decoder parks literals at the output tail); nothing outside the chunks is written on either path."""
    torch = torch_cuda
    src = corpus_mix(200_000, 41)
    base = [(src[:4099], 1), (src[100_000:116_385], -1), (src[20_000:90_000], 1), (src[199_000:199_255], -5),
            (src[5000:5000 + 140_000], 1)]
    valid = [np.frombuffer(expect(np.ascontiguousarray(c), lv), np.uint8) for c, lv in base]
    if O.have_ref():                             # (the bases are valid frames of their chunks, on the CPU)
        for (c, lv), f in zip(base, valid):
            r, out = O.decompress_chunks(f, np.array([len(f)]), len(c), "zstd", len(c))
            assert r == len(c) and (out == c).all()
    rng = np.random.default_rng(77)
    frames, sizes = [], []
    for m in range(200):
        j = m % len(base)
        f = valid[j].copy()
        if m % 4 == 3:                           # truncation
            f = f[: int(rng.integers(1, len(f)))]
        else:                                    # one byte changed (headers more often than the payload's middle)
            pos = int(rng.integers(0, min(len(f), 24))) if m % 4 == 0 else int(rng.integers(0, len(f)))
            f[pos] ^= int(rng.integers(1, 256))
        frames.append(f.tobytes())
        sizes.append(len(base[j][0]))
    st, got, offs, states = decode_frames(torch, frames, sizes, max(sizes), True)
    ust, ugot, uoffs, _ = decode_frames(torch, frames, sizes, max(sizes), False)
    assert (offs == uoffs).all()
    assert (st == ust).all(), [(i, int(st[i]), int(ust[i])) for i in np.flatnonzero(st != ust)[:8]]
    mask = np.zeros(len(got), bool)
    for i, s in enumerate(sizes):
        mask[offs[i]: offs[i] + s] = True
        if st[i] >= 0:
            assert (got[offs[i]: offs[i] + s] == ugot[offs[i]: offs[i] + s]).all(), f"frame {i}: bytes differ"
    assert (got[~mask] == 0xEE).all() and (ugot[~mask] == 0xEE).all(), "write outside the chunks"
    assert (st < 0).sum() >= 50
    assert set(states.tolist()) <= {SPLIT, LEGACY}


# ---- 5. an oversize chunk -----------------------------------------------------------------------------------------
def test_oversize_chunk_is_not_processed(torch_cuda):
    torch = torch_cuda
    maxb = 140000
    sizes = [3000, maxb + 1, maxb, 17000]        # entry 1 is one byte too large (and really that large)
    k = len(sizes)
    offs, total = layout(sizes)
    host = corpus_mix(total, 17)
    rc = L.RaggedCodec("zstd", maxb, k, 1, max_total_bytes=sum(sizes), split_decode=True)
    rc.compress(to_dev(torch, host), offs, sizes)
    check_batch(torch, rc, len(sizes), expected(host, offs, sizes, 1), skip={1})
    zt = split_bytes(maxb, k)
    buf = guarded_temp(torch, rc, zt)
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})    # (chunk 1's bytes count as outside: they keep their fill)
    assert int(st[1]) == -1
    assert bool((buf[zt:] == 0xEE).all())
    states = frame_states(rc, maxb, k)
    assert states.tolist() == [SPLIT] * k                     # (not processed: done, as far as the kernels care)
    f0, fsize, stride = region(maxb, k, 1)
    assert fsize == k * stride
    slot = [buf[f0 + i * stride: f0 + (i + 1) * stride] for i in range(k)]
    assert bool((slot[1] == 0xEE).all()), "the oversize chunk's temp slot was written"
    assert not bool((slot[0] == 0xEE).all()) and not bool((slot[2] == 0xEE).all())


# ---- 7. graph replay ----------------------------------------------------------------------------------------------
def test_graph_replay(torch_cuda):
    torch = torch_cuda
    level = 1
    sizes = [70000, 0, 13, 4099, 131073, 9]
    k = len(sizes)
    offs, total = layout(sizes)
    host = corpus_mix(total, 29)
    d_in = to_dev(torch, host)
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    rc = L.RaggedCodec("zstd", max(sizes), k, level, split_decode=True)
    assert rc.dtemp.numel() == split_bytes(max(sizes), k)
    d_src, _ = rc._arrays(d_in, offs, sizes, 16)
    d_dst, _ = rc._arrays(out, offs, sizes, 0)
    torch.cuda.synchronize()

    def pair():
        rc.compress_arrays(d_src, k)
        rc.decompress_arrays(d_dst, k)

    def check():
        torch.cuda.synchronize()
        _, _, packed = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level))
        got = out.cpu().numpy()
        assert (rc.status[:k].cpu().numpy() == np.array(sizes)).all()
        for o, s in zip(offs, sizes):
            assert (got[o: o + s] == host[o: o + s]).all()
        assert SPLIT in frame_states(rc, max(sizes), k).tolist()
        return packed.tobytes(), got.tobytes()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):       # captured on a non-default stream: one linear chain
        pair()
    replays = []
    for _ in range(2):
        for t in (out, rc.packed, rc.csizes, rc.offsets, rc.status, rc.dtemp):
            t.zero_()
        g.replay()
        replays.append(check())
    assert replays[0] == replays[1]


# ---- 8. d_offsets = NULL ------------------------------------------------------------------------------------------
def test_offsets_are_derived_into_the_split_temp(torch_cuda):
    torch = torch_cuda
    sizes = [70000, 5, 16385, 0, 131073, 4099]
    k, maxb = len(sizes), max(sizes)
    offs, total = layout(sizes)
    host = corpus_mix(total, 31)
    rc = L.RaggedCodec("zstd", maxb, k, 1, max_total_bytes=sum(sizes), split_decode=True)
    rc.compress(to_dev(torch, host), offs, sizes)
    torch.cuda.synchronize()
    want = rc.offsets[: k + 1].cpu().numpy()
    zt = split_bytes(maxb, k)
    buf = guarded_temp(torch, rc, zt)
    roundtrip(torch, rc, host, offs, sizes, csizes=rc.csizes, offsets=None)
    assert bool((buf[zt:] == 0xEE).all())
    o0, osize, _ = region(maxb, k, 0)
    assert (rc.dtemp[o0: o0 + osize].cpu().numpy().view(np.int64) == want).all()
    assert SPLIT in frame_states(rc, maxb, k).tolist()
