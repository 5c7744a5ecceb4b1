"""GPU: ragged zstd batches on the device API (include/lzbench_hip.h 3c, lzbench_amd.RaggedCodec("zstd")) --
per-chunk pointers and sizes against the CPU restatement and the reference build frame by frame, against the
uniform call, their guards, and the ragged decoder against reference frames and the uniform verdicts.
Run with -m gpu."""
import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
import gpu_batches as B
from gpu_batches import SLACK, check_batch, layout, roundtrip, to_dev, torch_cuda
from test_zstd_golden import arrays, cases, corpus
from zstd_ragged_inputs import EDGE_L2, EDGE_SIZES, codec_name, corpus_mix, edge_input, expect, expected

pytestmark = pytest.mark.gpu

ZSTD = L.LZH_CODEC_ZSTD
LEVELS = [1, -1, -5]


# ---- 1. edge sizes in one batch; 6. the round trip through the ragged decoder --------------------------------
@pytest.mark.parametrize("level", LEVELS + [2])
def test_edge_sizes_in_one_batch(torch_cuda, edge_input, level):
    torch = torch_cuda
    host, offs = edge_input
    sizes = EDGE_L2 if level == 2 else EDGE_SIZES
    offs = offs[: len(sizes)]                       # (the sizes up to 128 KiB are the first entries)
    assert sizes == EDGE_SIZES[: len(sizes)] and sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    rc = L.RaggedCodec(codec_name(level), max(sizes), len(sizes), level, max_total_bytes=sum(sizes))
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, packed = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level))
    assert int(cs[0]) == 9                          # the empty chunk's frame
    assert [int(c) for c in cs[1:4]] == [1 + 9, 6 + 9, 7 + 9]   # small chunks expand and are not stored raw
    roundtrip(torch, rc, host, offs, sizes)
    # once more with the decompress call's d_offsets = NULL: the offsets are scanned into temp
    roundtrip(torch, rc, host, offs, sizes, csizes=rc.csizes, offsets=None)


# ---- 2. equals the uniform call --------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, -5])
@pytest.mark.parametrize("chunk", [65536, 131072, 300000])
def test_equals_the_uniform_call(torch_cuda, chunk, level):
    torch = torch_cuda
    n = (1 << 20) + 333
    host = corpus_mix(n, 3)
    d_in = to_dev(torch, host, SLACK)
    dc = L.DeviceCodec(codec_name(level), n, chunk, level)
    dc.compress(d_in)
    sizes = L.chunk_sizes_for(n, chunk).astype(np.int64)
    offs = np.arange(len(sizes), dtype=np.int64) * chunk
    rc = L.RaggedCodec(codec_name(level), chunk, len(sizes), level, max_total_bytes=n)
    rc.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    k = len(sizes)
    assert dc.k == k
    assert torch.equal(rc.csizes[:k], dc.csizes) and torch.equal(rc.offsets[: k + 1], dc.offsets)
    total = dc.packed_total()
    assert rc.packed_total() == total and torch.equal(rc.packed[:total], dc.packed[:total])


# ---- 3. order and aliasing -------------------------------------------------------------------------------------
def test_order_and_aliasing(torch_cuda, edge_input):
    torch = torch_cuda
    host, offs = edge_input
    level = 1
    perm = np.random.default_rng(5).permutation(len(EDGE_SIZES))
    p_offs = np.concatenate([offs[perm], offs[[16, 16, 9]]])       # two entries at chunk 16's bytes, a third at 9's
    p_sizes = [EDGE_SIZES[i] for i in perm] + [EDGE_SIZES[16], EDGE_SIZES[16], EDGE_SIZES[9]]
    rc = L.RaggedCodec("zstd", max(EDGE_SIZES), len(p_sizes), level)
    rc.compress(to_dev(torch, host), p_offs, p_sizes)
    cs, of, packed = check_batch(torch, rc, len(p_sizes), expected(host, p_offs, p_sizes, level))
    k = len(p_sizes)
    assert packed[of[k - 3]: of[k - 2]].tobytes() == packed[of[k - 2]: of[k - 1]].tobytes()


# ---- 4. an oversize chunk; 5. guards ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, -1])
def test_oversize_chunk_is_not_processed(torch_cuda, level):
    torch = torch_cuda
    maxb = 140000                               # (two blocks: the second launch must skip the chunk as well)
    sizes = [3000, maxb + 1, maxb, 17]          # entry 1 is one byte too large (and really that large)
    offs, total = layout(sizes)
    host = corpus_mix(total, 17)
    rc = L.RaggedCodec(codec_name(level), maxb, len(sizes), level, max_total_bytes=sum(sizes))
    # the temp buffer is exactly the sizing answer, the packed buffer exactly max_packed; guard bytes on both sides
    G = 4096
    lib = L.lib()
    ct = lib.lzh_zstd_ragged_compress_temp_bytes(level, maxb, len(sizes))
    assert ct == rc.ctemp.numel()
    temp = torch.full((ct + 2 * G,), 0xEE, dtype=torch.uint8, device="cuda")
    packed = torch.full((rc.max_packed + 2 * G,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.ctemp, rc.packed = temp[G: G + ct], packed[G: G + rc.max_packed]
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, _ = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level), skip={1})
    assert int(cs[1]) == 0 and of[1] == of[2]
    assert bool((temp[:G] == 0xEE).all()) and bool((temp[G + ct:] == 0xEE).all()), "write outside the temp buffer"
    assert bool((packed[:G] == 0xEE).all()) and bool((packed[G + int(of[4]):] == 0xEE).all()), "write outside packed"
    # the oversize chunk's staging slot (slot 1) and scratch area (area 1) were not touched
    stride = lib.lzh_stage_stride(ZSTD, maxb)
    assert bool((temp[G + stride: G + 2 * stride] == 0xEE).all()), "the oversize chunk's staging slot was written"
    area = (ct - (len(sizes) * stride + 256) - 256) // len(sizes)      # (temp_layout.h chunk_temp: slots, gap, areas, gap)
    a0 = G + len(sizes) * stride + 256
    assert area > maxb and bool((temp[a0 + area: a0 + 2 * area] == 0xEE).all()), "the oversize chunk's scratch was written"
    assert not bool((temp[a0: a0 + area] == 0xEE).all()) and not bool((temp[a0 + 2 * area: a0 + 3 * area] == 0xEE).all())
    # decode side: the same entry reports -1 and writes nothing; its neighbours decode
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})
    assert int(st[1]) == -1


def test_temp_and_packed_cap_guards(torch_cuda):
    torch = torch_cuda
    level = 1
    sizes = [70000, 5, 16385, 0, 131073, 4099]
    offs, total = layout(sizes)
    host = corpus_mix(total, 31)
    rc = L.RaggedCodec("zstd", max(sizes), len(sizes), level, max_total_bytes=sum(sizes))
    d_in = to_dev(torch, host)
    rc.compress(d_in, offs, sizes)
    cs, of, full = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, level))
    k = len(sizes)
    # temp of exactly the sizing answers, followed by guard bytes that stay as they are (compress and decompress)
    G = 4096
    lib = L.lib()
    ct = lib.lzh_zstd_ragged_compress_temp_bytes(level, max(sizes), k)
    dt = lib.lzh_zstd_ragged_decompress_temp_bytes(max(sizes), k)
    ctemp = torch.full((ct + G,), 0xEE, dtype=torch.uint8, device="cuda")
    dtemp = torch.full((dt + G,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.ctemp, rc.dtemp = ctemp[:ct], dtemp[:dt]
    # a packed_cap below the total: chunks whose range would pass it are not written, the sizes are all reported
    cap = int(of[4]) + 100                       # inside chunk 4's frame
    big = torch.full((int(of[k]) + G,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.packed = big[:cap]
    rc.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    assert (rc.csizes[:k].cpu().numpy() == cs).all() and (rc.offsets[: k + 1].cpu().numpy() == of).all()
    assert rc.packed_total() > cap               # the caller learns that the output is incomplete
    got = big.cpu().numpy()
    assert (got[: of[4]] == full[: of[4]]).all(), "chunks below the cap"
    assert (got[cap:] == 0xEE).all(), "bytes past packed_cap were written"
    assert bool((ctemp[ct:] == 0xEE).all()), "write past the compress temp"
    # decode the complete output with the exact decompress temp, offsets scanned into it
    rc.packed = to_dev(torch, full, 256)
    roundtrip(torch, rc, host, offs, sizes, csizes=rc.csizes, offsets=None)
    assert bool((dtemp[dt:] == 0xEE).all()), "write past the decompress temp"


# ---- 7. reference frames the encoder never writes ---------------------------------------------------------------
def decode_frames(torch, frames, out_sizes, maxb):
    """frames (bytes each) as one ragged batch: (status, output canvas, output offsets)"""
    rc = L.RaggedCodec("zstd", maxb, len(frames), 1, max_total_bytes=sum(out_sizes))
    return B.decode_frames(torch, rc, frames, out_sizes)


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
    st, got, offs = decode_frames(torch, frames, sizes, max(sizes))
    mask = np.zeros(len(got), bool)
    for i, p in enumerate(parts):
        assert int(st[i]) == len(p), f"frame {i}: status {st[i]}"
        assert (got[offs[i]: offs[i] + len(p)] == p).all(), f"frame {i}: bytes differ"
        mask[offs[i]: offs[i] + len(p)] = True
    assert (got[~mask] == 0xEE).all()


# ---- 8. a raw-stored chunk on decode ----------------------------------------------------------------------------
def test_raw_stored_chunk_is_copied(torch_cuda):
    torch = torch_cuda
    raw = L.datagen("random", 4099, seed=2)      # csize == out_bytes: a copy, whatever the bytes are
    text = L.datagen("text", 9000, seed=4)
    st, got, offs = decode_frames(torch, [raw.tobytes(), expect(text, 1), raw[:7].tobytes()], [4099, 9000, 7], 9000)
    assert st.tolist() == [4099, 9000, 7]
    assert (got[offs[0]: offs[0] + 4099] == raw).all() and (got[offs[1]: offs[1] + 9000] == text).all()
    assert (got[offs[2]: offs[2] + 7] == raw[:7]).all()
    # (the encoder's side: a frame of incompressible bytes is size + 10 or more, a raw block in a frame, so the
    # rule only fires where a frame happens to have its chunk's size; test_edge_sizes_in_one_batch and
    # test_equals_the_uniform_call compare such frames with the restatement's and the uniform call's)


# ---- 9. malformed frames get the uniform verdicts -----------------------------------------------------------------
def test_malformed_frames_get_the_uniform_verdicts(torch_cuda):
    """Seeded single-byte mutations and truncations of valid frames: status and output equal those of
    lzh_decompress_async on the same frame alone with temp_bytes = 0 (its one-wave path).  Both sides are
    deterministic, bounds-checked decoders: verdict parity on fixed inputs."""
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
        if m % 4 == 3:                           # truncation
            f = f[: int(rng.integers(1, len(f)))]
        else:                                    # one byte changed (headers more often than the payload's middle)
            pos = int(rng.integers(0, min(len(f), 24))) if m % 4 == 0 else int(rng.integers(0, len(f)))
            f[pos] ^= int(rng.integers(1, 256))
        frames.append(f.tobytes())
        sizes.append(len(base[j][0]))
    k = len(frames)
    st, got, offs = decode_frames(torch, frames, sizes, max(sizes))
    # the uniform call, one frame at a time: same packed bytes at the same addresses, outputs at the same offsets
    lib = L.lib()
    packed = to_dev(torch, np.frombuffer(b"".join(frames), np.uint8), 256)
    csizes = torch.tensor([len(f) for f in frames], dtype=torch.int32, device="cuda")
    zero = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.full((len(got),), 0xEE, dtype=torch.uint8, device="cuda")
    status = torch.full((k,), -99, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    pos = 0
    for i, f in enumerate(frames):
        rc = lib.lzh_decompress_async(ZSTD, packed.data_ptr() + pos, packed.numel() - pos, csizes.data_ptr() + 4 * i,
                                      zero.data_ptr(), sizes[i], sizes[i], out.data_ptr() + int(offs[i]),
                                      status.data_ptr() + 4 * i, None, 0, stream)
        assert rc == 0
        pos += len(f)
    torch.cuda.synchronize()
    ust, uout = status.cpu().numpy(), out.cpu().numpy()
    assert (st == ust).all(), [(i, int(st[i]), int(ust[i])) for i in np.flatnonzero(st != ust)[:8]]
    assert (got == uout).all(), "outputs differ"
    assert (st < 0).sum() >= 50 and len(set(st[st < 0].tolist())) >= 1     # the mutations do reach the checks


# ---- 10. graph replay ---------------------------------------------------------------------------------------------
def test_graph_replay(torch_cuda):
    torch = torch_cuda
    level = 1
    sizes = [70000, 0, 13, 4099, 131073, 9]
    offs, total = layout(sizes)
    host = corpus_mix(total, 29)
    d_in = to_dev(torch, host)
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    rc = L.RaggedCodec("zstd", max(sizes), len(sizes), level)
    d_src, k = rc._arrays(d_in, offs, sizes, 16)
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
        return packed.tobytes()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):       # captured on a non-default stream
        pair()
    replays = []
    for _ in range(2):
        for t in (out, rc.packed, rc.csizes, rc.offsets, rc.status):
            t.zero_()
        g.replay()
        replays.append(check())
    assert replays[0] == replays[1]
