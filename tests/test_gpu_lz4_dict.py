"""GPU: LZ4 ragged batches with a shared dictionary (include/lzbench_hip.h 3d, RaggedCodec(dictionary=...)) against
the reference build's own LZ4_loadDict + LZ4_compress_fast_continue and LZ4_decompress_safe_usingDict
(tests/lz4_dict_ref.py), byte for byte.  Run with -m gpu."""
import numpy as np
import pytest

from gpu_batches import check_batch, layout, place, roundtrip, to_dev, torch_cuda
import lz4_dict_inputs as I
import lz4_dict_ref as R
import lzbench_amd as L
from lz_streams import Lz4Writer

pytestmark = pytest.mark.gpu

MAXB = 200000


def codec(torch, d: np.ndarray, maxb, k, acc=1, residue=0):
    """A RaggedCodec over dictionary d; residue: the dictionary pointer's address mod 4 (the codec's own copy is
    aligned: a second copy at that residue, 16 readable bytes after it, takes its place in the calls)."""
    rc = L.RaggedCodec("lz4fast", maxb, k, acc, dictionary=torch.from_numpy(d))
    if residue:
        assert rc.dictionary.data_ptr() % 4 == 0
        rc.dict_shifted = torch.zeros(len(d) + residue + 16, dtype=torch.uint8, device="cuda")
        rc.dict_shifted[residue: residue + len(d)].copy_(torch.from_numpy(d))
        rc._head["dict"] = rc.dict_shifted.data_ptr() + residue
    return rc


def ref_packed(d, parts, acc):
    """(packed, csizes) as the reference writes the batch, raw-store rule applied"""
    blocks = [R.packed(d, p, acc) for p in parts]
    cs = np.array([len(b) for b in blocks], np.int32)
    return np.frombuffer(b"".join(blocks), np.uint8), cs


@pytest.fixture(scope="module")
def matrix():
    parts = [c for _, c in I.chunks()]
    return (parts,) + place(parts)


@pytest.mark.parametrize("name,d", I.dictionaries(), ids=[n for n, _ in I.dictionaries()])
def test_every_dictionary_with_every_chunk(torch_cuda, matrix, name, d):
    R.need()
    torch = torch_cuda
    parts, host, offs, sizes = matrix
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    d_in = to_dev(torch, host)
    for acc in (1, 7):
        for residue in (0, 1):
            rc = codec(torch, d, MAXB, len(parts), acc, residue)
            rc.compress(d_in, offs, sizes)
            check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], acc))
            roundtrip(torch, rc, host, offs, sizes)
        # the reference's own streams, offsets derived on the device
        rp, rcs = ref_packed(d, parts, acc)
        roundtrip(torch, rc, host, offs, sizes, packed=to_dev(torch, rp, 256), csizes=torch.from_numpy(rcs).cuda())


@pytest.mark.parametrize("name", list(I.constructed()))
def test_constructed_cases(torch_cuda, name):
    R.need()
    torch = torch_cuda
    d, c = I.constructed()[name]
    host, offs, sizes = place([c, c[: len(c) // 2], c])
    parts = [host[o: o + s] for o, s in zip(offs, sizes)]
    for acc in (1, 7):
        rc = codec(torch, d, max(sizes), 3, acc, residue=acc % 2)
        rc.compress(to_dev(torch, host), offs, sizes)
        check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], acc))
        roundtrip(torch, rc, host, offs, sizes)


def test_small_json_records_compress_better_with_the_dictionary(torch_cuda):
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 65536)
    parts = [I.chunk("json", 1000), I.chunk("json", 4096)]
    host, offs, sizes = place(parts)
    d_in = to_dev(torch, host)
    rc = codec(torch, d, 4096, 2)
    rc.compress(d_in, offs, sizes)
    cs, _, _ = check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], 1))
    plain = L.RaggedCodec("lz4", 4096, 2)
    plain.compress(d_in, offs, sizes)
    torch.cuda.synchronize()
    pcs = plain.csizes[:2].cpu().numpy()
    print("with dictionary", cs, "alone", pcs)
    assert (cs < pcs).all()


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
    ct = L.lib().lzh_lz4_dict_compress_temp_bytes(len(d), maxb, 4)
    temp = torch.full((ct + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    rc.ctemp = temp[G: G + ct]
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, _ = check_batch(torch, rc, len(parts), lambda i: R.packed(d, parts[i], 1), skip={1})
    assert int(cs[1]) == 0 and of[1] == of[2]
    assert bool((temp[:G] == 0xA5).all()) and bool((temp[G + ct:] == 0xA5).all()), "write outside the temp buffer"
    stride = L.lib().lzh_stage_stride(L.LZH_CODEC_LZ4, maxb)
    assert bool((temp[G + stride: G + 2 * stride] == 0xA5).all()), "the oversize chunk's staging slot was written"
    st = roundtrip(torch, rc, host, offs, sizes, skip={1})
    assert int(st[1]) == -1


def test_packed_cap_one_byte_short(torch_cuda):
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 4095)
    parts = [I.chunk("json", 1000), I.chunk("text", 4096), I.chunk("json", 64)]
    host, offs, sizes = place(parts)
    _, rcs = ref_packed(d, parts, 1)
    total = int(rcs.sum())
    rc = codec(torch, d, 4096, 3)
    full = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    rc.packed = full[: total - 1]                       # one byte short: the last chunk does not fit
    rc.compress(to_dev(torch, host), offs, sizes)
    torch.cuda.synchronize()
    assert (rc.csizes[:3].cpu().numpy() == rcs).all()
    assert int(rc.offsets[3].item()) == total > rc.packed.numel()    # reported: the output is incomplete
    got = full.cpu().numpy()
    assert got[: total - int(rcs[2])].tobytes() == b"".join(R.packed(d, p) for p in parts[:2])
    assert (got[total - int(rcs[2]):] == 0x5A).all(), "a chunk past packed_cap was written"


def hand_streams(d: bytes):
    """[(name, stream, cap, expected bytes or None where the reference rejects)] from the stream writer"""
    D = len(d)
    tail = b"0123456789abcdefghijklmnopqrstuvwxyz"[:20]
    out = []
    lits = b"abc" if D + 3 <= 65535 else b""                            # (an offset has 16 bits)
    w = Lz4Writer(prefix=d).seq(lits, len(lits) + D, 8).last(tail)      # the dictionary's first byte
    out.append(("off=op+dict", w.finish(w.pos), w.pos, w.expected))
    if len(lits) + D + 1 <= 65535:
        w = Lz4Writer(prefix=d).seq(lits, len(lits) + D + 1, 8).last(tail)   # one before it
        cap = len(lits) + 8 + len(tail)
        out.append(("off=op+dict+1", w.finish(cap, valid=False), cap, None))
    # 5 literals, then 300 bytes from 7 before the dictionary's end: 7 of the dictionary, the 5 literals, then its
    # own output again and again (period 12)
    w = Lz4Writer(prefix=d).seq(b"LMNOP", 12, 300).last(tail)
    out.append(("cross-and-overlap", w.finish(w.pos), w.pos, w.expected))
    w = Lz4Writer().seq(b"no dictionary here", 7, 40).seq(b"xy", 1, 30).last(tail)
    out.append(("no-dictionary", w.finish(w.pos), w.pos, w.expected))
    return out


@pytest.mark.parametrize("dname", ["json-11", "json-4095", "text-65535"])
def test_hand_written_streams(torch_cuda, dname):
    R.need()
    torch = torch_cuda
    d = dict(I.dictionaries())[dname]
    cases = hand_streams(d.tobytes())
    caps = [c[2] for c in cases]
    offs, total = layout(caps)
    packed = np.frombuffer(b"".join(c[1] for c in cases), np.uint8)
    rcs = np.array([len(c[1]) for c in cases], np.int32)
    rc = codec(torch, d, max(caps), len(cases), residue=1)
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    rc.decompress(out, offs, caps, packed=to_dev(torch, packed, 256), csizes=torch.from_numpy(rcs).cuda())
    torch.cuda.synchronize()
    st, got = rc.status[: len(cases)].cpu().numpy(), out.cpu().numpy()
    for i, (name, s, cap, exp) in enumerate(cases):
        r, rb = R.decompress(d, s, cap)
        if exp is None:
            assert r < 0 and int(st[i]) < 0, (name, r, st[i])
        else:
            assert r == len(exp) and rb == exp, name              # the writer's model and the reference agree
            assert int(st[i]) == r and got[offs[i]: offs[i] + r].tobytes() == exp, (name, st[i])


def test_single_byte_corruptions_get_the_reference_verdicts(torch_cuda):
    R.need()
    torch = torch_cuda
    rng = np.random.default_rng(77)
    C = I.constructed()
    sources = [(I.dictionary("json", 4095), I.chunk("json", 1000)), (I.dictionary("text", 4095), I.chunk("text", 4096)),
               (C["tail40-cross"][0][-4095:], C["tail40-cross"][1])]
    # one dictionary per launch: the three sources in three launches of 100 corruptions each
    for d, c in sources:
        base = np.frombuffer(R.compress(d, c), np.uint8)
        assert len(base) != len(c)
        streams = []
        for _ in range(100):
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
        print(f"{len(streams)} corruptions of a {len(base)}-byte block: the reference accepts {accepted}")


def test_graph_replay(torch_cuda):
    R.need()
    torch = torch_cuda
    d = I.dictionary("json", 65536)
    parts = [I.chunk("json", 4096), I.chunk("text", 1000), I.chunk("json", 13), I.chunk("json", 0)]
    host, offs, sizes = place(parts)
    d_in = to_dev(torch, host)
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    rc = codec(torch, d, 4096, 4)
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
    for t in (out, rc.packed, rc.csizes, rc.offsets, rc.status):
        t.zero_()
    g.replay()
    assert (check() == eager).all()
