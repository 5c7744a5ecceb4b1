"""GPU: the LZ4 and snappy compress kernels on the parser events that tests/test_lzc_census.py pins -- the named
inputs (tests/lzc_inputs.py) through the uniform device call, the per-chunk row, the ragged and the compact ragged
call (every input at all four residues mod 4), as LZ4 frames with independent and linked blocks (one 4 MiB block, and linked 64 KiB blocks
for the inputs above 64 KiB; every acceleration the frame parameters hold) and as nvcomp containers, against the restatement byte for byte (itself the reference build's bytes on these inputs, CPU test),
with a round trip; and the parse kernel's own event counters (lzh_debug_lz4_stats) over the same inputs.  Every
comparison is exact.  The census of what ran is printed once.  Run with -m gpu.

Found by these inputs: `zeros600000` failed on every path before the kernel fix (2371 bytes where the reference
writes 2363).  The parse's slow count (slow_count, finish_match; lzbench_amd/csrc/lz4c.h) stopped after 1024
steps of 256 bytes, so a match ran no further than 262164 bytes past its seed where LZ4_count stops only at
matchlimit: the match was cut and a re-test sequence followed it.  `zeros16m` passes the same cap in the fused
kernel (chunks over 16 MiB).  The catch-up loops of the kernels that catch up in the parse (the fused kernel,
linked frames) had the same shape, 4096 steps of 64 bytes, which `accper21845`'s catch-up of 1.4 MB passes; that cap
was read in the code and lifted with the other, the input was not run before the fix.  In the linked-frame kernel
the catch-up's second step and beyond run on `accper99x140k` (6.3 KiB) as a frame of three linked blocks.  Both loops end at
matchlimit / at the anchor and the chunk's start by themselves; their step bounds are now out of any chunk's reach
(kCountSteps, kCatchupSteps).  The three inputs stay
here as the regression tests.

The kernel-side counters come from the records-only parse (the production parse kernel's instantiation): its
`sequences` equals the restatement's sequence count chunk by chunk; it does no catch-up (the emission kernel does),
so `catchup_slow` is not counted there and is not required."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import lzbench_amd as L
import lzc_census as Z
import lzc_inputs as I
import oracle_lib as O
from gpu_batches import check_batch, layout, roundtrip, to_dev, torch_cuda
from ragged_inputs import expected
from test_lzc_census import IDS, ROWS, census_of, data_of

pytestmark = pytest.mark.gpu

RAGGED_MAX = 16 << 20          # the ragged calls take chunks up to 16 MiB
FRAME_MAX = 4 << 20            # one 4 MiB block: the largest LZ4 frame block
_ran = Counter()               # the census of every chunk a test here compressed
_kernel = Counter()            # the parse kernel's own counters
STAT_NAMES = {0: "batches", 1: "collision_batches", 2: "slow_colliders", 3: "sequences", 4: "window_moved",
              5: "catchup_slow", 6: "count_slow", 9: "pside_from_memory", 12: "refills"}


def _expected(inp, level):
    """(packed bytes, csizes) of the row as one chunk, from the restatement's chunk loop (raw-store rule applied)"""
    d = data_of(inp)
    return O.compress_chunks(np.ascontiguousarray(d), I.codec_of(inp, level), len(d), level)


# ---- a. the uniform device call and the per-chunk row --------------------------------------------------------------
@pytest.mark.parametrize("inp,level", ROWS, ids=IDS)
def test_uniform_call_and_row(torch_cuda, inp, level):
    torch = torch_cuda
    d = data_of(inp)
    n, codec = len(d), I.codec_of(inp, level)
    out, cens = census_of(inp, level)
    exp, ecs = _expected(inp, level)
    dc = L.DeviceCodec(codec, n, n, level=level)
    dc.compress(to_dev(torch, d, 256))
    dc.decompress()
    torch.cuda.synchronize()
    total = dc.packed_total()
    assert int(dc.csizes[0].item()) == int(ecs[0]) and total == len(exp), (int(dc.csizes[0].item()), int(ecs[0]))
    assert dc.packed[:total].cpu().numpy().tobytes() == exp.tobytes(), "uniform call: bytes differ from the restatement"
    assert int(dc.status[0].item()) == n and (dc.out[:n].cpu().numpy() == d).all()
    # the row's compress function returns the compressor's own bytes (lzbench applies the raw-store rule itself)
    lib = L.lib()
    fn = {"lz4": "lz4", "lz4fast": "lz4fast", "snappy": "snappy"}[codec]
    lvl = L._row_level(codec, level)
    with L._Row(codec, n, lvl) as row:
        buf = np.zeros(L.get_compress_bound(n) + 64, np.uint8)
        src = np.ascontiguousarray(d)
        clen = getattr(lib, f"lzbench_hip_{fn}_compress")(src.ctypes.data, n, buf.ctypes.data, len(buf), lvl, 0, row.wm)
        assert clen == len(out) == inp.packed[level], (clen, len(out))
        assert buf[:clen].tobytes() == out, "per-chunk row: bytes differ from the restatement"
        back = np.zeros(n + L.PAD_SIZE, np.uint8)
        base = "snappy" if codec == "snappy" else "lz4"
        dlen = getattr(lib, f"lzbench_hip_{base}_decompress")(buf.ctypes.data, clen, back.ctypes.data, n, lvl, 0, row.wm)
        assert dlen == n and (back[:n] == d).all()
    _ran.update(cens)


# ---- b. the ragged calls: every input of a (codec, level) in one batch, four times, so at every residue mod 4 ------
def _groups():
    g = {}
    for inp, level in ROWS:
        if len(data_of(inp)) <= RAGGED_MAX:
            g.setdefault((I.codec_of(inp, level), level), []).append(inp)
    return sorted(g.items(), key=lambda kv: (kv[0][0], kv[0][1]))


@pytest.mark.parametrize("compact", [False, True], ids=["slots", "compact"])
def test_ragged_batches(torch_cuda, compact):
    torch = torch_cuda
    for (codec, level), inps in _groups():
        parts = [data_of(i) for i in inps for _ in range(4)]
        sizes = [len(p) for p in parts]
        offs, total = layout(sizes)
        assert all({int(offs[4 * j + r]) % 4 for r in range(4)} == {0, 1, 2, 3} for j in range(len(inps)))
        host = np.zeros(total, np.uint8)
        for o, p in zip(offs, parts):
            host[o: o + len(p)] = p
        rc = L.RaggedCodec(codec, max(sizes), len(sizes), level, max_total_bytes=sum(sizes), compact=compact)
        rc.compress(to_dev(torch, host), offs, sizes)
        cs, _, _ = check_batch(torch, rc, len(sizes), expected(host, offs, sizes, codec, level))
        roundtrip(torch, rc, host, offs, sizes)
        for j, i in enumerate(inps):
            if i.packed[level] < len(data_of(i)):        # (else stored raw: check_batch held it to the rule)
                assert int(cs[4 * j]) == i.packed[level], (i.name, level)
            _ran.update(census_of(i, level)[1])


# ---- c. framed: LZ4 frames (independent and linked blocks) and nvcomp containers ------------------------------------
# (the frame parameters carry accelerations up to 255)
FRAME_ROWS = [(i, lv) for i, lv in ROWS if i.codec == "lz4" and lv <= 255 and len(data_of(i)) <= FRAME_MAX]


@pytest.mark.parametrize("inp,level", FRAME_ROWS, ids=[f"{i.name}-l{lv}" for i, lv in FRAME_ROWS])
def test_frames_and_containers(torch_cuda, inp, level):
    d = np.ascontiguousarray(data_of(inp))
    n = len(d)
    acc = (level << 8) if level > 1 else 0
    cases = [("lz4f", "lz4frame", 0x07 | acc), ("lz4f", "lz4frame", 0x87 | acc)]
    if n > 65536:     # several 64 KiB blocks: linked, they go through the linked-frame kernel (a frame of one block,
        cases.append(("lz4f", "lz4frame", 0x84 | acc))      # as above, is independent and takes the chunk codec's)
    if level == 1:
        cases.append(("nvlz4", "nvcomp_lz4", 5))
    for ocodec, name, params in cases:
        exp, ecs = O.compress_chunks(d, ocodec, n, params)
        packed, cs = L.compress_chunks(d, name, n, level=params)
        assert (cs == ecs).all() and len(packed) == len(exp), (name, hex(params), cs, ecs)
        assert packed.tobytes() == exp.tobytes(), (name, hex(params))
        assert (L.decompress_chunks(packed, cs, n, name, n) == d).all()
    _ran.update(census_of(inp, level)[1])


# ---- d. the parse kernel's own counters ------------------------------------------------------------------------------
def test_kernel_side_census(torch_cuda):
    torch = torch_cuda
    f = L.lib().lzh_debug_lz4_stats
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for inp, level in ROWS:
        d = data_of(inp)
        n = len(d)
        if inp.codec != "lz4" or n > RAGGED_MAX:
            continue
        codec = I.codec_of(inp, level)
        dc = L.DeviceCodec(codec, n, n, level=level)
        d_in = to_dev(torch, d, 256)
        st = torch.zeros(32, dtype=torch.int64, device="cuda")
        assert f(d_in.data_ptr(), n, d_in.numel(), n, level, dc.ctemp.data_ptr(), dc.csizes.data_ptr(), st.data_ptr(),
                 torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        v = st.cpu().tolist()
        want = census_of(inp, level)[1]["lz4/sequences"]
        assert v[3] == want, f"{inp.name} at acceleration {level}: the kernel counts {v[3]} sequences, the parser {want}"
        for i, name in STAT_NAMES.items():
            _kernel[name] += v[i]
    for name in ("batches", "collision_batches", "slow_colliders", "sequences", "window_moved", "count_slow",
                 "pside_from_memory"):
        assert _kernel[name] > 0, (name, dict(_kernel))


def test_zz_print_census():
    """(last in the file) the classes the tests above ran, and the ones they did not"""
    print("\ncompressor census of this file's GPU runs:", dict(sorted(_ran.items())))
    print("parse kernel counters:", dict(_kernel))
    print("not run here:", sorted(set(Z.ALL_CLASSES) - set(k for k in _ran if _ran[k])))
