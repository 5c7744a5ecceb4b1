"""GPU: the level-3 (double-fast) compress kernels on the parser events that tests/test_zstd_dfast_census.py pins --
the named inputs (tests/zstd_dfast_inputs.py) through the uniform device call and the per-chunk row, and all but the
multi-megabyte one through one ragged and one compact ragged batch in which each input appears four times, so at
every residue mod 4 (the parse reads 8 bytes at arbitrary positions).  Every result is compared byte for byte with
the committed digests (tests/golden/zstd_dfast_census_golden.json: the reference build's frames) and with the
reference build itself where it is present, and decoded back by the GPU decoders.  The census of what ran is printed
once.  Run with -m gpu.

Found by these inputs: nothing.  Every input reproduced the reference's bytes on every path on the first run; the
host walk's invariant counters say that the walk never reads below the frame's first byte, so the max(pos, 0) clamps
of WaveEnv::r32 / r64 do not act on any of these inputs."""
import hashlib
import json
import os
from collections import Counter

import numpy as np
import pytest

import lzbench_amd as L
import oracle_lib as O
import zstd_dfast_census as D
import zstd_dfast_inputs as I
from test_gpu_zstd_dfast_ragged import decode_both, frames, result
from gpu_batches import layout, sha, to_dev, torch_cuda

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD, "zstd_dfast_census_golden.json")) as _f:
    GOLDEN = {c["name"]: c for c in json.load(_f)["cases"]}
SMALL = [i for i in I.INPUTS if i.name != I.FAR]
_ran = Counter()               # the census of every frame a test here compressed (needs the host walk's library)
_data = {}


def data_of(inp):
    if inp.name not in _data:
        d = np.ascontiguousarray(inp.make())
        assert sha(d) == GOLDEN[inp.name]["input_sha256"] and len(d) == GOLDEN[inp.name]["n"], inp.name
        _data[inp.name] = d
    return _data[inp.name]


def count(inp):
    if D.have_lib():
        d = data_of(inp)                       # (with the reference build: which blocks confirm their repcodes)
        confirm = [t == "cmp" for t in D.block_types(D.ref_frame(d))] if O.have_ref() else None
        _ran.update(D.walk(d, confirm)[0])


def check_one(inp, packed: bytes, what):
    """one chunk's packed bytes against the digest, and against the reference build where present"""
    g = GOLDEN[inp.name]
    assert len(packed) == g["packed_bytes"], (inp.name, what, len(packed), g["packed_bytes"])
    assert hashlib.sha256(packed).hexdigest() == g["packed_sha256"], (inp.name, what)
    if O.have_ref():
        d = data_of(inp)
        ep, _ = O.compress_chunks(d, "zstd", len(d), 3, use_ref=True)
        assert packed == ep.tobytes(), (inp.name, what)


def test_fixture_lists_every_input():
    assert list(GOLDEN) == [i.name for i in I.INPUTS]


def uniform_and_row(torch, inp):
    d = data_of(inp)
    n = len(d)
    dc = L.DeviceCodec("zstd_dfast", n, n, level=3)
    d_in = to_dev(torch, d, 256)
    dc.compress(d_in)
    dc.decompress()
    torch.cuda.synchronize()
    total = dc.packed_total()
    assert int(dc.csizes[0].item()) == total
    assert sha(dc.csizes.cpu().numpy().astype("<u8")) == GOLDEN[inp.name]["csizes_sha256"]
    check_one(inp, dc.packed[:total].cpu().numpy().tobytes(), "uniform call")
    assert int(dc.status[0].item()) == n and torch.equal(dc.out[:n], d_in[:n])
    # the row's compress function returns the compressor's own frame (lzbench applies the raw-store rule itself)
    lib = L.lib()
    wm = lib.lzbench_hip_zstd_dfast_init(n, 3, 1)
    assert wm
    try:
        out = np.zeros(L.get_compress_bound(n) + 64, np.uint8)
        clen = lib.lzbench_hip_zstd_dfast_compress(d.ctypes.data, n, out.ctypes.data, len(out), 3, 0, wm)
        frame = out[:clen].tobytes()
        if clen != n and total != n:                   # (neither stored raw by the chunk loop)
            check_one(inp, frame, "per-chunk row")
        elif O.have_ref():
            assert frame == D.ref_frame(d), (inp.name, "per-chunk row")
        back = np.zeros(n + 64, np.uint8)
        assert lib.lzbench_hip_zstd_decompress(out.ctypes.data, clen, back.ctypes.data, n, 0, 0, wm) == n
        assert (back[:n] == d).all()
    finally:
        lib.lzbench_hip_deinit(wm)
    count(inp)


# ---- a. the uniform device call and the per-chunk row --------------------------------------------------------------
@pytest.mark.parametrize("inp", SMALL, ids=lambda i: i.name)
def test_uniform_call_and_row(torch_cuda, inp):
    uniform_and_row(torch_cuda, inp)


def test_uniform_call_and_row_multi_megabyte(torch_cuda):
    """the 2.5 MiB input, the only one whose window slides; through the uniform call and the row only"""
    uniform_and_row(torch_cuda, I.BY_NAME[I.FAR])


# ---- b. the ragged calls: every small input in one batch, four times, so at every residue mod 4 ---------------------
@pytest.mark.parametrize("mode", ["uniform", "compact"])
def test_ragged_batches(torch_cuda, mode):
    torch = torch_cuda
    parts = [data_of(i) for i in SMALL for _ in range(4)]
    sizes = [len(p) for p in parts]
    offs, total = layout(sizes)
    assert all({int(offs[4 * j + r]) % 4 for r in range(4)} == {0, 1, 2, 3} for j in range(len(SMALL)))
    host = np.full(total, 0x5A, np.uint8)
    for o, p in zip(offs, parts):
        host[o: o + len(p)] = p
    rc = L.RaggedCodec("zstd_dfast", max(sizes), len(sizes), level=3, max_total_bytes=sum(sizes),
                       compact_scratch=mode == "compact")
    rc.compress(to_dev(torch, host), offs, sizes)
    got = frames(*result(torch, rc, len(sizes)))
    for j, inp in enumerate(SMALL):
        for r in range(4):
            check_one(inp, got[4 * j + r], f"{mode} ragged batch, copy {r}")
        count(inp)
    decode_both(torch, rc, host, offs, sizes)


def test_zz_print_census():
    """(last in the file) the classes the tests above ran, and the ones they did not"""
    if not D.have_lib():
        print("\nthe host walk's library (oracle/libzdfcensus.so) is not built: no census")
        return
    print("\nlevel-3 parser census of this file's GPU runs:", dict(sorted(_ran.items())))
    print("not run here:", sorted(set(D.classes()) - set(k for k in _ran if _ran[k])))
