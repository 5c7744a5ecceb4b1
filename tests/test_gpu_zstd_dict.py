"""GPU: zstd ragged batches with a shared dictionary (include/lzbench_hip.h 3f, RaggedCodec("zstd", dictionary=...))
against the reference build's own ZSTD_compress_usingDict and ZSTD_decompress_usingDict (tests/zstd_dict_ref.py),
byte for byte; and the decoder on the hand-built frames of tests/zstd_dict_frames.py, whose expected bytes are that
module's pure-Python model (tests/test_zstd_dict_frames.py holds the model to the reference).  Run with -m gpu."""
import numpy as np
import pytest

from gpu_batches import check_batch, decode_frames, layout, place, roundtrip, to_dev, torch_cuda
import lzbench_amd as L
import zstd_dict_frames as F
import zstd_dict_inputs as I
import zstd_dict_ref as R

pytestmark = pytest.mark.gpu


def codec(torch, d: np.ndarray, maxb, k, level=1, residue=0):
    """A RaggedCodec over dictionary d; residue: the dictionary pointer's address mod 4 (the codec's own copy is
    aligned: a second copy at that residue, 16 readable bytes after it, takes its place in the calls)."""
    rc = L.RaggedCodec("zstd", maxb, k, level, dictionary=torch.from_numpy(d))
    if residue:
        assert rc.dictionary.data_ptr() % 4 == 0
        rc.dict_shifted = torch.zeros(len(d) + residue + 16, dtype=torch.uint8, device="cuda")
        rc.dict_shifted[residue: residue + len(d)].copy_(torch.from_numpy(d))
        rc._head["dict"] = rc.dict_shifted.data_ptr() + residue
    return rc


@pytest.mark.parametrize("name,kind,d", I.dictionaries(), ids=[n for n, _, _ in I.dictionaries()])
def test_every_dictionary_with_every_chunk(torch_cuda, name, kind, d):
    """the matrix: every chunk size and kind, levels 1 and -3, chunk and dictionary pointers over all residues"""
    R.need()
    torch = torch_cuda
    parts = [c for _, c in I.chunks(kind, len(d))]
    host, offs, sizes = place(parts)
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    d_in = to_dev(torch, host)
    for j, level in enumerate(I.LEVELS):
        for residue in (2 * j, 2 * j + 1):
            rc = codec(torch, d, 131072, len(parts), level, residue)
            rc.compress(d_in, offs, sizes)
            check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], level))
            roundtrip(torch, rc, host, offs, sizes)


@pytest.mark.parametrize("name", list(I.constructed()))
def test_constructed_cases(torch_cuda, name):
    R.need()
    torch = torch_cuda
    d, c = I.constructed()[name]
    host, offs, sizes = place([c, c[: len(c) // 2], c])
    parts = [host[o: o + s] for o, s in zip(offs, sizes)]
    for level in I.LEVELS:
        rc = codec(torch, d, max(sizes), 3, level, residue=level % 4)
        rc.compress(to_dev(torch, host), offs, sizes)
        check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], level))
        roundtrip(torch, rc, host, offs, sizes)


def test_reference_frames_of_other_levels_decode(torch_cuda):
    """frames no encoder here writes: the reference at levels 3, 5 and 19 with the dictionary; and frames written
    without a dictionary"""
    R.need()
    torch = torch_cuda
    for kind, nd in (("json", 65536), ("text", 4095)):
        d = I.dictionary(kind, nd)
        parts = [I.chunk(kind, s) for s in (300, 1000, 4099, 16384, 70000)]
        host, offs, sizes = place(parts)
        rc = codec(torch, d, 131072, len(parts), residue=1)
        for level in (3, 5, 19):
            rp, rcs = R.packed_batch(d, parts, level)
            roundtrip(torch, rc, host, offs, sizes, packed=to_dev(torch, rp, 256), csizes=torch.from_numpy(rcs).cuda())
        rp, rcs = R.packed_batch(d, parts, 1, plain=True)
        roundtrip(torch, rc, host, offs, sizes, packed=to_dev(torch, rp, 256), csizes=torch.from_numpy(rcs).cuda())


def test_offset_one_past_the_dictionary_is_an_error(torch_cuda):
    """a sequence whose offset is pos + dict_bytes reaches the dictionary's first byte; with the dictionary one byte
    shorter at its front the same sequence asks for pos + dict_bytes + 1: -1, as the reference"""
    R.need()
    torch = torch_cuda
    d, c = I.constructed()["catchup-dict-start"]
    frame = R.compress(d, c, 1)
    assert R.decompress(d, frame, len(c)) == (len(c), c.tobytes())
    assert R.decompress(d[1:], frame, len(c))[0] < 0
    offs, total = layout([len(c)])
    for dd, want in ((d, len(c)), (d[1:], -1)):
        rc = codec(torch, np.ascontiguousarray(dd), len(c), 1)
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        rc.decompress(out, offs, [len(c)], packed=to_dev(torch, np.frombuffer(frame, np.uint8), 256),
                      csizes=torch.tensor([len(frame)], dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert int(rc.status[0].item()) == want
        if want > 0:
            assert out.cpu().numpy()[offs[0]: offs[0] + len(c)].tobytes() == c.tobytes()


def test_single_byte_corruptions_get_the_reference_verdicts(torch_cuda):
    R.need()
    torch = torch_cuda
    rng = np.random.default_rng(79)
    sources = [(I.dictionary("json", 4096), I.chunk("json", 1000), 3), (I.dictionary("text", 65536), I.chunk("text", 4099), 5),
               (I.dictionary("json", 65536), I.chunk("json", 4099), 19)]
    for d, c, level in sources:
        base = np.frombuffer(R.compress(d, c, level), np.uint8)
        assert len(base) != len(c)
        streams = []
        for _ in range(200):
            s = base.copy()
            at = int(rng.integers(0, len(s)))
            s[at] ^= int(rng.integers(1, 256))
            streams.append(s)
        caps = [len(c)] * len(streams)
        offs, total = layout(caps)
        rc = codec(torch, d, len(c), len(streams))
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        rc.decompress(out, offs, caps, packed=to_dev(torch, np.concatenate(streams), 256),
                      csizes=torch.full((len(streams),), len(base), dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        st, got = rc.status[: len(streams)].cpu().numpy(), out.cpu().numpy()
        accepted = 0
        for i, s in enumerate(streams):
            r, rb = R.decompress(d, s.tobytes(), len(c))
            assert (r < 0) == (int(st[i]) < 0), f"corruption {i}: reference {r}, GPU {st[i]}"
            if r >= 0:
                accepted += 1
                assert int(st[i]) == r and got[offs[i]: offs[i] + r].tobytes() == rb, f"corruption {i}"
        print(f"{len(streams)} corruptions of a {len(base)}-byte frame: the reference accepts {accepted}")


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
    ct = L.lib().lzh_zstd_dict_compress_temp_bytes(1, len(d), maxb, 4)
    temp = torch.full((ct + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    rc.ctemp = temp[G: G + ct]
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, _ = check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], 1), skip={1})
    assert int(cs[1]) == 0 and of[1] == of[2]
    assert bool((temp[:G] == 0xA5).all()) and bool((temp[G + ct:] == 0xA5).all()), "write outside the temp buffer"
    stride = L.lib().lzh_stage_stride(L.LZH_CODEC_ZSTD, maxb)
    assert bool((temp[G + stride: G + 2 * stride] == 0xA5).all()), "the oversize chunk's staging slot was written"
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})
    assert int(st[1]) == -1


def test_packed_cap_one_byte_short(torch_cuda):
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 4095)
    parts = [I.chunk("json", 1000), I.chunk("text", 4099), I.chunk("json", 64)]
    host, offs, sizes = place(parts)
    _, rcs = R.packed_batch(d, parts, 1)
    total = int(rcs.sum())
    rc = codec(torch, d, 4099, 3)
    full = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    rc.packed = full[: total - 1]                       # one byte short: the last chunk does not fit
    rc.compress(to_dev(torch, host), offs, sizes)
    torch.cuda.synchronize()
    assert (rc.csizes[:3].cpu().numpy() == rcs).all()
    assert int(rc.offsets[3].item()) == total > rc.packed.numel()    # reported: the output is incomplete
    got = full.cpu().numpy()
    assert got[: total - int(rcs[2])].tobytes() == b"".join(R.packed(d, p) for p in parts[:2])
    assert (got[total - int(rcs[2]):] == 0x5A).all(), "a chunk past packed_cap was written"


def test_decode_without_offsets_and_equal_bytes_through_the_c_abi(torch_cuda):
    """NULL d_offsets on decode (derived from d_csizes in temp), and the C call itself next to RaggedCodec"""
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 4096)
    parts = [I.chunk("json", 1000), I.chunk("json", 0), I.chunk("text", 300), I.rand(64, 3)]
    host, offs, sizes = place(parts)
    d_in = to_dev(torch, host)
    rc = codec(torch, d, 1000, 4, -3)
    rc.compress(d_in, offs, sizes)
    cs, of, packed = check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], -3))
    roundtrip(torch, rc, host, offs, sizes, csizes=rc.csizes)          # offsets=None: scanned on the device
    # the same through the C ABI with buffers of this test's own
    lib = L.lib()
    arr, k = rc._arrays(d_in, offs, sizes, 16)
    ct = lib.lzh_zstd_dict_compress_temp_bytes(-3, len(d), 1000, 4)
    temp = torch.zeros(ct, dtype=torch.uint8, device="cuda")
    pk = torch.zeros(rc.packed.numel(), dtype=torch.uint8, device="cuda")
    cs2 = torch.zeros(4, dtype=torch.int32, device="cuda")
    of2 = torch.zeros(5, dtype=torch.int64, device="cuda")
    r = lib.lzh_zstd_compress_ragged_dict_async(-3, rc.dictionary.data_ptr(), len(d), arr[0].data_ptr(), arr[1].data_ptr(), k,
                                                1000, pk.data_ptr(), pk.numel(), cs2.data_ptr(), of2.data_ptr(),
                                                temp.data_ptr(), ct, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert r == 0 and (cs2.cpu().numpy() == cs).all() and (of2.cpu().numpy() == of).all()
    assert (pk[: int(of[4])].cpu().numpy() == packed).all()


def test_small_json_records_pack_smaller_with_the_dictionary(torch_cuda):
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 65536)
    parts = I.records("json", 512, 1024)
    host, offs, sizes = place(parts)
    d_in = to_dev(torch, host)
    rc = codec(torch, d, 1100, 512)
    rc.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    with_dict = rc.packed_total()
    plain = L.RaggedCodec("zstd", 1100, 512, 1)
    plain.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    alone = plain.packed_total()
    ref_dict = int(R.packed_batch(d, parts, 1)[1].sum())
    ref_alone = int(R.packed_batch(d, parts, 1, plain=True)[1].sum())
    print(f"512 JSON records, {sum(sizes)} bytes: {with_dict} with the dictionary, {alone} alone")
    assert with_dict == ref_dict and alone == ref_alone
    assert with_dict < alone
    roundtrip(torch, rc, host, offs, sizes)


# ---- the hand-built frames (tests/zstd_dict_frames.py): every path of a sequence whose source is the dictionary --
@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_hand_frames_decode(torch_cuda, residue):
    """one batch of every accepting frame; the expected bytes are the pure-Python model's"""
    torch = torch_cuda
    d = F.dictionary()
    acc = F.accepting()
    frames, caps = [f for _, f, _, _ in acc], [len(c) for _, _, c, _ in acc]
    rc = codec(torch, d, max(caps), len(acc), residue=residue)
    st, got, offs = decode_frames(torch, rc, frames, caps)
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    mask = np.zeros(len(got), bool)
    bad = []
    for i, (name, _, content, _) in enumerate(acc):
        o = int(offs[i])
        mask[o: o + caps[i]] = True
        if int(st[i]) != len(content):
            bad.append(f"{name}: status {st[i]}, content {len(content)}")
        elif got[o: o + caps[i]].tobytes() != content:
            diff = np.flatnonzero(got[o: o + caps[i]] != np.frombuffer(content, np.uint8))
            bad.append(f"{name}: {len(diff)} bytes differ, the first at {diff[0]}")
    assert not bad, "; ".join(bad)
    assert (got[~mask] == 0xEE).all(), "the decoder wrote outside the chunks"


def test_hand_frames_rejected(torch_cuda):
    """one call with the dictionary a byte shorter at its front: the frame that copies the whole dictionary now asks
    for a byte before it, and a dictionary ID other than 0 names another dictionary; nothing outside a chunk's own
    range is written"""
    torch = torch_cuda
    d = F.dictionary()
    assert len({cut for _, cut in F.REJECTS}) == 1
    short = np.ascontiguousarray(d[F.REJECTS[0][1]:])
    byname = {n: (f, c) for n, f, c, _ in F.frames()}
    frames, caps = [byname[n][0] for n, _ in F.REJECTS], [len(byname[n][1]) for n, _ in F.REJECTS]
    assert all(F.expected(n, short)[0] < 0 for n, _ in F.REJECTS)
    rc = codec(torch, short, max(caps), len(frames), residue=1)
    st, got, offs = decode_frames(torch, rc, frames, caps)
    assert all(int(s) < 0 for s in st), st
    mask = np.zeros(len(got), bool)
    for o, s in zip(offs, caps):
        mask[int(o): int(o) + s] = True
    assert (got[~mask] == 0xEE).all(), "a rejected frame wrote outside its chunk"


def test_reserved_mode_bits_on_the_plain_decoder(torch_cuda):
    """today's documented difference: the ragged zstd decoder without a dictionary refuses a reserved bit of the
    sequence-modes byte, the dictionary decoder (test_hand_frames_decode) gives the reference's verdict"""
    torch = torch_cuda
    byname = {n: (f, c) for n, f, c, _ in F.frames()}
    frames = [byname[n][0] for n in F.NEEDS_NO_DICTIONARY]
    caps = [len(byname[n][1]) for n in F.NEEDS_NO_DICTIONARY]
    rc = L.RaggedCodec("zstd", max(caps), len(frames), 1)
    st, got, offs = decode_frames(torch, rc, frames, caps)
    assert all(int(s) < 0 for s in st), st
    # the same frame with the bit cleared decodes: the bit alone is what the decoder refuses
    twin, content = F.reserved_plain_cleared()
    assert content == byname["reserved-bit0-plain"][1] and len(twin) == len(frames[0])
    assert sum(a != b for a, b in zip(twin, frames[0])) == 1
    clean = [twin]
    st, got, offs = decode_frames(torch, rc, clean, caps)
    for i, n in enumerate(F.NEEDS_NO_DICTIONARY):
        assert int(st[i]) == caps[i] and got[offs[i]: offs[i] + caps[i]].tobytes() == byname[n][1], n


@pytest.mark.parametrize("level", [-1, -2, -4, -5])
def test_the_other_levels(torch_cuda, level):
    """levels -1, -2, -4 and -5 (targetLength, the parse's step): the constructed pairs and three chunks of one text
    dictionary, byte for byte against the reference, and back"""
    R.need()
    torch = torch_cuda
    dt = I.dictionary("text", 4095)
    batches = [(d, [c]) for d, c in I.constructed().values()]
    batches.append((dt, [I.chunk("text", s) for s in (300, 4099, 16385)]))
    for j, (d, parts) in enumerate(batches):
        host, offs, sizes = place(parts)
        rc = codec(torch, d, max(sizes), len(parts), level, residue=j % 4)
        rc.compress(to_dev(torch, host), offs, sizes)
        check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], level))
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
        check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], 1))
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
