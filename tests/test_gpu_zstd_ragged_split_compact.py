"""GPU: ragged zstd batches through the split decoder in the compact temp layout (include/lzbench_hip.h 3g,
lzbench_amd.RaggedCodec("zstd", ..., split_decode=True, compact_decode=True)): statuses and bytes are those of the
one-wave decoder and of 3c's split call, nothing outside the chunks or past the sizing answer is written, the
placement in temp equals its host mirror, and the frame states tell which decoder finished each frame.
Run with -m gpu."""
import numpy as np
import pytest

import lzbench_amd as L
import zstd_hand_frames as H
from test_zstd_golden import arrays, cases, corpus
import gpu_batches as B
from gpu_batches import layout, roundtrip, to_dev, torch_cuda
from zstd_ragged_inputs import codec_name, corpus_mix, expect
from test_gpu_zstd_ragged_split import EDGE_SIZES, GUARD, LEGACY, SPLIT, guarded_temp, small_bytes, split_bytes
from test_gpu_zstd_ragged_split import decode_frames as decode_frames_3c

pytestmark = pytest.mark.gpu


def compact_bytes(total, maxb, k):
    return L.lib().lzh_zstd_ragged_decompress_split_compact_temp_bytes(total, maxb, k)


def regions(total, maxb, k):
    """[(offset, size)] of the 11 regions of the compact temp, and its total"""
    v = np.zeros(23, np.uint64)
    assert L.lib().lzh_debug_zstd_ragged_split_compact_layout(total, maxb, k, v.ctypes.data) == 0
    return [(int(v[2 * i]), int(v[2 * i + 1])) for i in range(11)], int(v[22])


def mirror(sizes, maxb, total):
    k = len(sizes)
    sz = np.array(sizes, np.uint64)
    ao, jo, ins = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.uint8)
    assert L.lib().lzh_debug_zstd_ragged_split_compact_slots(sz.ctypes.data, k, maxb, total, ao.ctypes.data, jo.ctypes.data,
                                                             ins.ctypes.data) == 0
    return ao, jo, ins


def read(rc, reg, dtype, count):
    off, size = reg
    return rc.dtemp[off: off + size].cpu().numpy().view(dtype)[:count]


def states(rc, total, maxb, k):
    return read(rc, regions(total, maxb, k)[0][3], np.int32, k)


def codec(level, maxb, k, total, name=None):
    return L.RaggedCodec(name or codec_name(level), maxb, k, level, max_total_bytes=total, split_decode=True,
                         compact_decode=True)


# ---- 1. edge sizes in one batch, every hook ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_input():
    offs, total = layout(EDGE_SIZES)
    host = corpus_mix(total, 23)
    i = EDGE_SIZES.index(131072)                   # a text chunk: four Huffman streams of over 4096 symbols (hufpar)
    host[offs[i]: offs[i] + 131072] = L.datagen("text", 131072, seed=9)
    return host, offs


@pytest.mark.parametrize("level,name", [(1, None), (-5, None), (3, "zstd_dfast")])
def test_edge_sizes_in_one_batch(torch_cuda, edge_input, level, name):
    torch = torch_cuda
    host, offs = edge_input
    sizes, k, maxb, total = EDGE_SIZES, len(EDGE_SIZES), 300000, sum(EDGE_SIZES)
    rc = codec(level, maxb, k, total, name)
    zt, dt = compact_bytes(total, maxb, k), small_bytes(maxb, k)
    assert rc.dtemp.numel() == zt > dt > 0
    rc.compress(to_dev(torch, host), offs, sizes)
    torch.cuda.synchronize()
    lib = L.lib()
    big = [i for i, s in enumerate(sizes) if s >= 16384]
    hooks = {"default": None, "huf8": (lib.lzh_debug_zstd_huf_sections, 8, 0), "nopar": (lib.lzh_debug_zstd_hufpar, 0, 1),
             "legacy": (lib.lzh_debug_zstd_legacy, 1, 0)}
    for hname, hook in hooks.items():
        buf = guarded_temp(torch, rc, zt)
        try:
            if hook:
                assert hook[0](hook[1]) == 0
            roundtrip(torch, rc, host, offs, sizes)
        finally:
            if hook:
                hook[0](hook[2])
        assert bool((buf[zt:] == 0xEE).all()), f"{hname}: write past the compact temp"
        st = states(rc, total, maxb, k)
        if hname == "legacy":
            assert (st.view(np.uint32) == 0xEEEEEEEE).all(), "legacy hook: the split kernels ran"
        else:
            print(hname, level, "frame states", st.tolist())
            assert all(int(st[i]) == SPLIT for i in big), (hname, st.tolist())
            assert set(st.tolist()) <= {SPLIT, LEGACY}
    for nbytes in (dt, zt - 1):                    # the small temp, and one byte short: one wave a frame
        buf = guarded_temp(torch, rc, nbytes)
        roundtrip(torch, rc, host, offs, sizes)
        assert bool((buf[nbytes:] == 0xEE).all()), "write past the temp"
        off, size = regions(total, maxb, k)[0][3]
        if off + size <= nbytes:
            assert bool((buf[off: off + size] == 0xEE).all()), "temp below the sizing answer: the split kernels ran"


# ---- 2, 3. a skewed batch; the same with a broken promise ---------------------------------------------------------
SKEW = [4096] * 64
SKEW[5] = 2 << 20


@pytest.fixture(scope="module")
def skew_input():
    offs, total = layout(SKEW)
    host = corpus_mix(total, 51)
    host[offs[5]: offs[5] + SKEW[5]] = L.datagen("text", SKEW[5], seed=3)
    return host, offs


def test_skewed_batch(torch_cuda, skew_input):
    torch = torch_cuda
    host, offs = skew_input
    sizes, k, maxb, total = SKEW, len(SKEW), max(SKEW), sum(SKEW)
    rc = codec(1, maxb, k, total)
    zt = compact_bytes(total, maxb, k)
    assert rc.dtemp.numel() == zt and zt * 10 < split_bytes(maxb, k)
    rc.compress(to_dev(torch, host), offs, sizes)
    buf = guarded_temp(torch, rc, zt)
    roundtrip(torch, rc, host, offs, sizes)
    assert bool((buf[zt:] == 0xEE).all())
    st = states(rc, total, maxb, k)
    print("skewed batch: frame states", st.tolist())
    assert set(st.tolist()) <= {SPLIT, LEGACY}
    reg, _ = regions(total, maxb, k)
    ao, jo, ins = mirror(sizes, maxb, total)
    assert ins.all()
    area_sz, job_cnt = read(rc, reg[7], np.uint32, k), read(rc, reg[8], np.uint32, k)
    area_off, job_off = read(rc, reg[9], np.uint64, k + 1), read(rc, reg[10], np.uint64, k + 1)
    assert (area_off[:k] == ao).all() and (job_off[:k] == jo).all()
    assert (np.diff(area_off) == area_sz).all() and (np.diff(job_off) == job_cnt).all()
    assert (job_cnt == np.array([(s + 131071) // 131072 + 1 for s in sizes])).all()


def test_broken_promise_costs_speed_only(torch_cuda, skew_input):
    torch = torch_cuda
    host, offs = skew_input
    sizes, k, maxb = SKEW, len(SKEW), max(SKEW)
    rc = codec(1, maxb, k, sum(sizes))
    rc.compress(to_dev(torch, host), offs, sizes)
    torch.cuda.synchronize()
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    d, _ = rc._arrays(out, offs, sizes, 0)
    half = sum(sizes) // 2
    rc.max_total = half                            # (the promise the decode call is handed)
    zt = compact_bytes(half, maxb, k)
    buf = guarded_temp(torch, rc, zt)
    rc.decompress_arrays(d, k)
    torch.cuda.synchronize()
    assert bool((buf[zt:] == 0xEE).all())
    st, got = rc.status[:k].cpu().numpy(), out.cpu().numpy()
    for i, s in enumerate(sizes):
        assert int(st[i]) == s and (got[offs[i]: offs[i] + s] == host[offs[i]: offs[i] + s]).all(), i
    _, _, ins = mirror(sizes, maxb, half)
    zs = states(rc, half, maxb, k)
    print("broken promise: in_split", ins.tolist(), "states", zs.tolist())
    assert not ins.all()
    assert all(int(zs[i]) == LEGACY for i in range(k) if not ins[i])   # (mirror 0: not finished by the split kernels)


# ---- 4. an oversize chunk ------------------------------------------------------------------------------------------
def test_oversize_chunk_is_not_processed(torch_cuda):
    torch = torch_cuda
    maxb = 140000
    sizes = [3000, maxb + 1, maxb, 17000]
    k, total = len(sizes), sum(sizes)
    offs, n = layout(sizes)
    host = corpus_mix(n, 17)
    rc = codec(1, maxb, k, total)
    rc.compress(to_dev(torch, host), offs, sizes)
    zt = compact_bytes(total, maxb, k)
    buf = guarded_temp(torch, rc, zt)
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})
    assert int(st[1]) == -1
    assert bool((buf[zt:] == 0xEE).all())
    assert states(rc, total, maxb, k).tolist() == [SPLIT] * k
    reg, _ = regions(total, maxb, k)
    area_off = read(rc, reg[9], np.uint64, k + 1)
    assert int(area_off[2]) == int(area_off[1])   # (no area)
    assert read(rc, reg[8], np.uint32, k)[1] == 0


# ---- 5, 6. frames from elsewhere -----------------------------------------------------------------------------------
def decode_frames(torch, frames, out_sizes, maxb):
    k, total = len(frames), sum(out_sizes)
    rc = codec(1, maxb, k, total)
    nbytes = compact_bytes(total, maxb, k)
    assert nbytes > 0 and rc.dtemp.numel() == nbytes
    buf = guarded_temp(torch, rc, nbytes)
    st, got, offs = B.decode_frames(torch, rc, frames, out_sizes)
    assert bool((buf[nbytes:] == 0xEE).all()), "write past the temp"
    return st, got, offs, states(rc, total, maxb, k)


def test_frames_the_encoders_do_not_write(torch_cuda):
    """Hand-built frames and the reference's (level 3 and 19, raw and RLE blocks), each with its exact size.  A
    frame of more blocks than ceil(n / 128 KiB) + 1, its own block slots, goes to the one-wave kernel here; only the
    range of the states is asserted (they are printed, with the names of the frames at LEGACY).
    On an MI355X two of the 20 frames went LEGACY, both of more blocks than their two slots: the hand-built
    `rle_block` (100,133 bytes in 4 blocks) and frame 0 of the reference's `text_b128_l19` (131,072 bytes, which
    level 19 splits into 3 blocks).  The other 18 ended SPLIT."""
    torch = torch_cuda
    A = arrays()
    names, frames, parts = [], [], []
    for name, frame, content in H.hand_frames():
        names.append("hand/" + name)
        frames.append(bytes(frame))
        parts.append(np.frombuffer(bytes(content), np.uint8))
    for c in cases():
        data, packed, cs = corpus(c), A[c["name"] + "/packed"], A[c["name"] + "/csizes"]
        pos = 0
        for i, s in enumerate(cs):
            names.append("%s/%d" % (c["name"], i))
            frames.append(packed[pos: pos + int(s)].tobytes())
            parts.append(data[i * c["chunk"]: (i + 1) * c["chunk"]])
            pos += int(s)
    sizes = [len(p) for p in parts]
    maxb = max(max(sizes), 16384)
    st, got, offs, zs = decode_frames(torch, frames, sizes, maxb)
    ust, ugot, uoffs, _ = decode_frames_3c(torch, frames, sizes, maxb, False)
    assert (st == ust).all() and (offs == uoffs).all()
    mask = np.zeros(len(got), bool)
    for i, p in enumerate(parts):
        assert int(st[i]) == len(p), f"frame {i}: status {st[i]}"
        assert (got[offs[i]: offs[i] + len(p)] == p).all(), f"frame {i}: bytes differ"
        mask[offs[i]: offs[i] + len(p)] = True
    assert (got == ugot).all()
    assert (got[~mask] == 0xEE).all(), "write outside the chunks"
    print("frames from elsewhere: states", zs.tolist())
    print("frames from elsewhere: LEGACY", [(names[i], sizes[i]) for i in range(len(zs)) if int(zs[i]) == LEGACY])
    assert set(zs.tolist()) <= {SPLIT, LEGACY}


def test_malformed_frames_get_the_one_wave_verdicts(torch_cuda):
    torch = torch_cuda
    src = corpus_mix(200_000, 41)
    base = [(src[:4099], 1), (src[100_000:116_385], -1), (src[20_000:90_000], 1), (src[199_000:199_255], -5),
            (src[5000:5000 + 140_000], 1)]
    valid = [np.frombuffer(expect(np.ascontiguousarray(c), lv), np.uint8) for c, lv in base]
    rng = np.random.default_rng(77)
    frames, sizes = [], []
    for m in range(200):
        j = m % len(base)
        f = valid[j].copy()
        if m % 4 == 3:
            f = f[: int(rng.integers(1, len(f)))]
        else:
            pos = int(rng.integers(0, min(len(f), 24))) if m % 4 == 0 else int(rng.integers(0, len(f)))
            f[pos] ^= int(rng.integers(1, 256))
        frames.append(f.tobytes())
        sizes.append(len(base[j][0]))
    st, got, offs, zs = decode_frames(torch, frames, sizes, max(sizes))
    ust, ugot, uoffs, _ = decode_frames_3c(torch, frames, sizes, max(sizes), False)
    assert (offs == uoffs).all()
    assert (st == ust).all(), [(i, int(st[i]), int(ust[i])) for i in np.flatnonzero(st != ust)[:8]]
    mask = np.zeros(len(got), bool)
    for i, s in enumerate(sizes):
        mask[offs[i]: offs[i] + s] = True
        if st[i] >= 0:
            assert (got[offs[i]: offs[i] + s] == ugot[offs[i]: offs[i] + s]).all(), f"frame {i}: bytes differ"
    assert (got[~mask] == 0xEE).all(), "write outside the chunks"
    assert (st < 0).sum() >= 50
    assert set(zs.tolist()) <= {SPLIT, LEGACY}


# ---- 7. equal chunks: 3c's split call --------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [131072, 16384])
def test_equal_chunks_equal_the_uniform_slot_call(torch_cuda, chunk):
    torch = torch_cuda
    sizes = [chunk] * 8
    k, total = 8, 8 * chunk
    offs, n = layout(sizes)
    host = corpus_mix(n, 61)
    assert compact_bytes(total, chunk, k) == split_bytes(chunk, k) + 2 * 256 + 2 * 256   # (the four arrays)
    rc = codec(1, chunk, k, total)
    d_in = to_dev(torch, host)
    rc.compress(d_in, offs, sizes)
    st = roundtrip(torch, rc, host, offs, sizes)
    zs = states(rc, total, chunk, k)
    ru = L.RaggedCodec("zstd", chunk, k, 1, max_total_bytes=total, split_decode=True)
    ru.compress(d_in, offs, sizes)
    ust = roundtrip(torch, ru, host, offs, sizes)
    v = np.zeros(16, np.uint64)
    assert L.lib().lzh_debug_zstd_ragged_split_layout(chunk, k, v.ctypes.data) == 0
    uzs = ru.dtemp[int(v[6]): int(v[6]) + 4 * k].cpu().numpy().view(np.int32)
    assert (st == ust).all() and zs.tolist() == uzs.tolist() == [SPLIT] * k


# ---- 8. graph capture -------------------------------------------------------------------------------------------------
def test_graph_replay(torch_cuda):
    torch = torch_cuda
    sizes = [70000, 0, 13, 4099, 131073, 9]
    k, total = len(sizes), sum(sizes)
    offs, n = layout(sizes)
    hosts = [corpus_mix(n, 29), corpus_mix(n, 30)]
    d_in = to_dev(torch, hosts[0])
    out = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = codec(1, max(sizes), k, total)
    d_src, _ = rc._arrays(d_in, offs, sizes, 16)
    d_dst, _ = rc._arrays(out, offs, sizes, 0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):       # one linear chain: no more than the default queues
        rc.compress_arrays(d_src, k)
        rc.decompress_arrays(d_dst, k)
    for host in (hosts[1], hosts[0]):
        d_in[: len(host)].copy_(torch.from_numpy(host))
        for t in (out, rc.packed, rc.csizes, rc.offsets, rc.status, rc.dtemp):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (rc.status[:k].cpu().numpy() == np.array(sizes)).all()
        for o, s in zip(offs, sizes):
            assert (got[o: o + s] == host[o: o + s]).all()
        assert SPLIT in states(rc, total, max(sizes), k).tolist()


# ---- 9. the Python flag -----------------------------------------------------------------------------------------------
def test_python_flag(torch_cuda):
    torch = torch_cuda
    sizes = [20000, 5, 70000]
    offs, n = layout(sizes)
    host = corpus_mix(n, 7)
    rc = L.RaggedCodec("zstd", 70000, 3, 1, max_total_bytes=sum(sizes), split_decode=True, compact_decode=True)
    assert rc.dtemp.numel() == compact_bytes(sum(sizes), 70000, 3)
    rc.compress(to_dev(torch, host), offs, sizes)
    roundtrip(torch, rc, host, offs, sizes)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd", 70000, 3, 1, compact_decode=True)
    with pytest.raises(ValueError):
        L.RaggedCodec("lz4", 70000, 3, 1, compact_decode=True)
    with pytest.raises(ValueError):
        L.RaggedCodec("zstd", 70000, 3, 1, split_decode=True, compact_decode=True,
                      dictionary=torch.zeros(64, dtype=torch.uint8, device="cuda"))
