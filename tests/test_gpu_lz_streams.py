"""GPU: the LZ4 and snappy decoders on valid streams that no encoder of this project writes (tests/lz_streams.py:
the named cases with their limit pairs, the generated streams, the LZ4 HC fixture) -- through each of the three
output-window kernels, the ragged decoder, the snappy fragment split in its test mode and off, and, wrapped as LZ4
frames (independent and linked blocks) and nvcomp containers, the frame decoders.  All streams of one capacity go
through one decompress call per path.  Every comparison is exact: a status is negative exactly when the case is
built to be rejected, otherwise it is the model's size and the bytes are the model's; the expected values are the
writers' byte models, which tests/test_lz_streams.py pins to the restatement and the reference decoders.  The census
union (tests/lz_census.py) of what ran is printed once.  Run with -m gpu.

Found by these streams: an LZ4 match at an offset under 64 that is no power of two and longer than the output window
less that offset (the generated stream random-65536-2: offset 62, 10061 bytes, first wrong byte 4096 into the match
under the 4 KiB window) decoded wrong with a success status.  owin::SinkT::match (lzbench_amd/csrc/decode_win.h)
read such a match's bytes from the one period before it for its whole length, and from KW - offset bytes on the match
itself had come round the window onto that period.  Powers of two hid it: there the bytes that come round are the
ones they replace, so runs of one byte never showed it.  The cases long-overlap-match@KW stay as its tests."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import lz_census as Z
import lz_streams as S
import oracle_lib as O
import lzbench_amd as L
from gpu_batches import to_dev, torch_cuda
from test_lz_streams import frame_verdict, hc_fixture, reference

pytestmark = pytest.mark.gpu
WINDOWS = [4096, 8192, 16384]
NAME = {"lz4f": "lz4frame", "nvlz4": "nvcomp_lz4"}

_ran = Counter()          # the census of every accepted stream a test here decoded


def _hook(name, restype=C.c_int):
    f = getattr(L.lib(), name)
    f.restype = restype
    f.argtypes = [C.c_int]
    return f


_batches = {}


def batches(codec):
    """{cap: [(name, stream, model output, expect_ok)]}: the named cases, the generated streams and (LZ4, capacity
    16384) the HC fixture"""
    if codec not in _batches:
        b = {}
        for c in S.CASES:
            if c.codec == codec:
                b.setdefault(c.cap, []).append((c.name, c.stream, c.out, c.ok))
        for cd, cap, lst in S.random_streams():
            if cd == codec:
                b[cap] += [(f"random-{cap}-{i}", s, o, True) for i, (s, o) in enumerate(lst)]
        if codec == "lz4":
            b[16384] = [("hc-" + m["name"], s, d.tobytes(), True) for m, s, d in hc_fixture()]
        if O.have_ref():       # the reference decoders first: a case they judge otherwise is a wrong case
            for cap, items in b.items():
                for name, s, o, ok in items:
                    r, got = reference(codec, s, cap)
                    assert (r >= 0) == ok and (not ok or got == o), f"the reference disagrees on {name}: the case is wrong"
        _batches[codec] = b
    return _batches[codec]


def decode_uniform(torch, codec, cap, streams):
    """the streams as the chunks of one DeviceCodec.decompress call (capacity cap each) -> (statuses, outputs)"""
    k = len(streams)
    dc = L.DeviceCodec(codec, k * cap, cap)
    dc.out.zero_()
    dc.decompress(packed=to_dev(torch, np.frombuffer(b"".join(streams), np.uint8), 256),
                  csizes=torch.tensor([len(s) for s in streams], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    return dc.status[:k].cpu().numpy(), dc.out[: k * cap].cpu().numpy().reshape(k, cap)


def check(items, status, out_of, what):
    """status[i] < 0 exactly for the rejected cases; else the model's size and bytes"""
    for i, (name, _, want, ok) in enumerate(items):
        st = int(status[i])
        assert (st < 0) == (not ok), f"{what} {name}: status {st}, expected {'a size' if ok else 'a rejection'}"
        if ok:
            assert st == len(want), f"{what} {name}: size {st}, model {len(want)}"
            assert out_of(i)[:st].tobytes() == want, f"{what} {name}: bytes differ from the model"


def note(codec, cap, items):
    for _, s, _, ok in items:
        if ok:
            _ran.update(Z.census(codec, s, cap))


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_window_kernels(torch_cuda, codec, window):
    force = _hook("lzh_debug_force_decode_window")
    try:
        assert force(window) == 0
        for cap, items in sorted(batches(codec).items()):
            st, out = decode_uniform(torch_cuda, codec, cap, [s for _, s, _, _ in items])
            check(items, st, lambda i: out[i], f"window {window} cap {cap}")
            if window == WINDOWS[0]:
                note(codec, cap, items)
    finally:
        force(0)


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_ragged_decoder(torch_cuda, codec):
    """every stream of every capacity as one ragged batch: outputs at all residues mod 4, nothing written outside"""
    torch = torch_cuda
    items = [(f"{cap}/{n}", s, o, ok, cap) for cap, lst in sorted(batches(codec).items()) for n, s, o, ok in lst]
    sizes = [cap for *_, cap in items]
    offs, pos = [], 0
    for i, n in enumerate(sizes):
        pos += 5 + (i % 4 - (pos + 5)) % 4
        offs.append(pos)
        pos += n
    total = pos + 64
    rc = L.RaggedCodec(codec, max(sizes), len(sizes), max_total_bytes=sum(sizes))
    out = torch.full((total,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.decompress(out, offs, sizes, packed=to_dev(torch, np.frombuffer(b"".join(s for _, s, *_ in items), np.uint8), 256),
                  csizes=torch.tensor([len(s) for _, s, *_ in items], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    st = rc.status[: len(sizes)].cpu().numpy()
    got = out.cpu().numpy()
    check([it[:4] for it in items], st, lambda i: got[offs[i]: offs[i] + sizes[i]], "ragged")
    mask = np.zeros(total, bool)
    for o, n in zip(offs, sizes):
        mask[o: o + n] = True
    assert (got[~mask] == 0xEE).all(), "write outside the chunks"


@pytest.mark.parametrize("mode", [0, 2])
def test_snappy_split_modes(torch_cuda, mode):
    """two-fragment chunks with the split off and in its test mode: the same bytes either way; in the test mode the
    split finishes exactly the streams that fill the chunk, start a tag at 65536 and copy nothing across it"""
    split, done = _hook("lzh_debug_snappy_split"), _hook("lzh_debug_snappy_split_done", C.c_longlong)
    cap = 131072
    items = batches("snappy")[cap]
    clean = 0
    for _, s, o, ok in items:
        if ok and len(o) == cap:
            c = Z.snappy(s, cap)[0]
            clean += bool(c["snappy/tag-at-fragment"]) and not c["snappy/copy/cross-fragment"]
    assert clean >= 8 and sum(ok and len(o) == cap for _, _, o, ok in items) - clean >= 8
    try:
        assert split(mode) == 0
        assert done(1) >= 0
        st, out = decode_uniform(torch_cuda, "snappy", cap, [s for _, s, _, _ in items])
        finished = done(0)
    finally:
        split(1)
    check(items, st, lambda i: out[i], f"split mode {mode}")
    assert finished == (clean if mode == 2 else 0)


@pytest.mark.parametrize("codec", ["lz4f", "nvlz4"])
def test_frame_decoders(torch_cuda, codec):
    """the full-size LZ4 blocks as frames of two blocks: independent, linked (block 2 starts with matches that begin
    in block 1 and run into it) and nvcomp containers; verdicts and bytes as the restatement's"""
    frames = [f for f in S.frames() if f.codec == codec]
    part = frames[0].part
    items = []
    for f in frames:
        r, got = frame_verdict(f)
        assert (r == part) == (f.out is not None) and (f.out is None or got == f.out), f.name
        items.append((f.name, f.frame, f.out or b"", f.out is not None))
    st, out = decode_uniform(torch_cuda, NAME[codec], part, [f.frame for f in frames])
    check(items, st, lambda i: out[i], NAME[codec])


def test_zz_print_census():
    """(last in the file) the classes the tests above ran"""
    from test_lz_streams import linked_block_census
    _ran.update(linked_block_census())
    print("\nLZ4 / snappy census of this file's GPU runs:", dict(sorted(_ran.items())))
    print("not run here:", sorted(set(Z.LZ4_CLASSES + Z.SNAPPY_CLASSES) - set(k for k in _ran if _ran[k])))
