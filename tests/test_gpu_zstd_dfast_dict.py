"""GPU: zstd level-3 ragged batches with a shared dictionary (include/lzbench_hip.h 3h,
RaggedCodec("zstd_dfast_dict", level=3, dictionary=...)) against the reference build's own ZSTD_compress_usingDict at
level 3 (tests/zstd_dict_ref.py), byte for byte, and back through 3f's decoder.  Run with -m gpu."""
import numpy as np
import pytest

import lzbench_amd as L
import zstd_dfast_dict_inputs as K
import zstd_dict_inputs as I
import zstd_dict_ref as R
from gpu_batches import check_batch, place, roundtrip, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
LEVEL = 3


def codec(torch, d: np.ndarray, maxb, k, residue=0):
    """A level-3 RaggedCodec over dictionary d; residue: the dictionary pointer's address mod 4 (a second copy at that
    residue, 16 readable bytes after it, takes the aligned copy's place in the calls)."""
    rc = L.RaggedCodec("zstd_dfast_dict", maxb, k, LEVEL, dictionary=torch.from_numpy(d))
    assert rc._crec.symbol == "lzh_zstd_dfast_compress_ragged_dict_async"
    assert rc._drec.symbol == "lzh_zstd_decompress_ragged_dict_async"
    if residue:
        assert rc.dictionary.data_ptr() % 4 == 0
        rc.dict_shifted = torch.zeros(len(d) + residue + 16, dtype=torch.uint8, device="cuda")
        rc.dict_shifted[residue: residue + len(d)].copy_(torch.from_numpy(d))
        rc._head["dict"] = rc.dict_shifted.data_ptr() + residue
    return rc


@pytest.mark.parametrize("name,kind,d", I.dictionaries(), ids=[n for n, _, _ in I.dictionaries()])
def test_every_dictionary_with_every_chunk(torch_cuda, name, kind, d):
    """the matrix: every chunk size and kind in one batch, chunk pointers over all residues"""
    R.need()
    torch = torch_cuda
    parts = [c for _, c in I.chunks(kind, len(d))]
    host, offs, sizes = place(parts)
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    rc = codec(torch, d, 131072, len(parts), residue=len(d) % 4)
    rc.compress(to_dev(torch, host), offs, sizes)
    check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], LEVEL))
    roundtrip(torch, rc, host, offs, sizes)


@pytest.mark.parametrize("name", list(K.constructed()))
def test_constructed_pairs(torch_cuda, name):
    R.need()
    torch = torch_cuda
    d, c = K.pairs()[name]
    host, offs, sizes = place([c, c[: len(c) // 2], c])
    parts = [host[o: o + s] for o, s in zip(offs, sizes)]
    rc = codec(torch, d, max(sizes), 3, residue=len(name) % 4)
    rc.compress(to_dev(torch, host), offs, sizes)
    check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], LEVEL))
    roundtrip(torch, rc, host, offs, sizes)


def test_oversize_chunk_is_not_processed(torch_cuda):
    R.need()
    torch = torch_cuda
    d = I.dictionary("text", 4095)
    maxb = 5000
    src = L.datagen("text", 20000, seed=17)
    parts = [src[:3000], src[3000: 3000 + maxb + 1], src[9000: 9000 + maxb], src[15000: 15017]]
    host, offs, sizes = place(parts)
    rc = codec(torch, d, maxb, 4)
    G = 4096
    lib = L.lib()
    ct = lib.lzh_zstd_dfast_dict_compress_temp_bytes(LEVEL, len(d), maxb, 4)
    temp = torch.full((ct + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    rc.ctemp = temp[G: G + ct]
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, _ = check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], LEVEL), skip={1})
    assert int(cs[1]) == 0 and of[1] == of[2]
    assert bool((temp[:G] == 0xA5).all()) and bool((temp[G + ct:] == 0xA5).all()), "write outside the temp buffer"
    stride = lib.lzh_stage_stride(L.LZH_CODEC_ZSTD, maxb)
    assert bool((temp[G + stride: G + 2 * stride] == 0xA5).all()), "the oversize chunk's staging slot was written"
    # its scratch area: after the 4 staging slots (256-aligned, 256 spare bytes), areas of one stride each
    recs = (4 * stride + 255) // 256 * 256 + 256
    rstride = (ct - recs - 256 - (lib.lzh_zstd_dfast_dict_compress_temp_bytes(LEVEL, len(d), maxb, 0) - 512)) // 4
    assert rstride > 0 and rstride % 256 == 0
    assert bool((temp[G + recs + rstride: G + recs + 2 * rstride] == 0xA5).all()), \
        "the oversize chunk's scratch area was written"
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})
    assert int(st[1]) == -1


def test_packed_cap_one_byte_short(torch_cuda):
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 4095)
    parts = [I.chunk("json", 1000), I.chunk("text", 4099), I.chunk("json", 64)]
    host, offs, sizes = place(parts)
    _, rcs = R.packed_batch(d, parts, LEVEL)
    total = int(rcs.sum())
    rc = codec(torch, d, 4099, 3)
    full = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    rc.packed = full[: total - 1]                       # one byte short: the last chunk does not fit
    rc.compress(to_dev(torch, host), offs, sizes)
    torch.cuda.synchronize()
    assert (rc.csizes[:3].cpu().numpy() == rcs).all()
    assert int(rc.offsets[3].item()) == total > rc.packed.numel()    # reported: the output is incomplete
    got = full.cpu().numpy()
    assert got[: total - int(rcs[2])].tobytes() == b"".join(R.packed(d, p, LEVEL) for p in parts[:2])
    assert (got[total - int(rcs[2]):] == 0x5A).all(), "a chunk past packed_cap was written"


def test_small_chunks_and_the_other_decoder(torch_cuda):
    """empty chunks and chunks under 7 bytes (the plain path); and the frames of a batch decode through a level-1
    dictionary codec as well: the decoder does not depend on the level that wrote the frame"""
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 4096)
    parts = [I.chunk("json", 0), I.chunk("json", 1), I.chunk("text", 6), I.chunk("json", 7), I.chunk("json", 1000),
             I.chunk("json", 0), I.rand(5, 3), I.chunk("text", 300)]
    host, offs, sizes = place(parts)
    rc = codec(torch, d, 1000, len(parts), residue=3)
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, packed = check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], LEVEL))
    assert int(cs[0]) == 9 and int(cs[5]) == 9, "an empty chunk is the 9-byte frame"
    for i in (1, 2, 6):
        assert packed[of[i]: of[i + 1]].tobytes() == R.packed_plain(parts[i], LEVEL), "under 7 bytes: the plain call's bytes"
    roundtrip(torch, rc, host, offs, sizes)
    other = L.RaggedCodec("zstd", 1000, len(parts), level=1, dictionary=torch.from_numpy(d))
    roundtrip(torch, other, host, offs, sizes, packed=rc.packed, csizes=rc.csizes, offsets=rc.offsets)


def test_json_records_pack_smaller_than_at_level_1(torch_cuda):
    """256 JSON records of about 1 KiB with a 64 KiB dictionary: level 3 against 3f's level-1 call (the reference's own
    two sizes for these inputs: asserted equal to the GPU's, and level 3 the smaller)"""
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 65536)
    parts = I.records("json", 256, 1024)
    host, offs, sizes = place(parts)
    d_in = to_dev(torch, host)
    ref3, ref1 = int(R.packed_batch(d, parts, 3)[1].sum()), int(R.packed_batch(d, parts, 1)[1].sum())
    rc = codec(torch, d, 1100, 256)
    rc.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    at3 = rc.packed_total()
    one = L.RaggedCodec("zstd", 1100, 256, 1, dictionary=torch.from_numpy(d))
    one.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    at1 = one.packed_total()
    print(f"256 JSON records, {sum(sizes)} bytes: {at3} at level 3, {at1} at level 1 (reference {ref3}, {ref1})")
    assert at3 == ref3 and at1 == ref1
    assert at3 < at1
    roundtrip(torch, rc, host, offs, sizes)


def test_zz_graph_replay(torch_cuda):
    """last: one capture and two replays of compress plus decode; every launch is on one stream, so the graph is a
    chain"""
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 65536)
    parts = [I.chunk("json", 4099), I.chunk("text", 1000), I.chunk("json", 9), I.chunk("json", 0)]
    host, offs, sizes = place(parts)
    d_in = to_dev(torch, host)
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    rc = codec(torch, d, 4099, 4)
    d_src, k = rc._arrays(d_in, offs, sizes, 16)
    d_dst, _ = rc._arrays(out, offs, sizes, 0)
    torch.cuda.synchronize()

    def pair():
        rc.compress_arrays(d_src, k)
        rc.decompress_arrays(d_dst, k)

    def check():
        torch.cuda.synchronize()
        check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], LEVEL))
        got = out.cpu().numpy()
        assert (rc.status[:k].cpu().numpy() == np.array(sizes)).all()
        for o, s in zip(offs, sizes):
            assert (got[o: o + s] == host[o: o + s]).all()
        return rc.packed[: rc.packed_total()].cpu().numpy().copy()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair()
    eager = check()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair()
    for _ in range(2):
        for t in (out, rc.packed, rc.csizes, rc.offsets, rc.status):
            t.zero_()
        g.replay()
        assert (check() == eager).all()
