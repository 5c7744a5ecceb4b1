"""GPU: ragged LZ4 frames (include/lzbench_hip.h 3i) through RaggedCodec("lz4frame").  Compression byte for byte
against the restatement's LZ4F_compressFrame per chunk (tests/lz4f_ragged_cases.py; the raw-store rule at frame
level) and against the uniform call; decoding of its own frames, of the restatement's independent and linked frames
and of corrupted frames against the restatement's LZ4F_decompress."""
import numpy as np
import pytest

import lz4f_ragged_cases as R
import lzbench_amd as L
from gpu_batches import (assert_roundtrip, check_batch, decode_frames, layout, place, to_dev,  # noqa: F401
                         torch_cuda)

pytestmark = pytest.mark.gpu
MAXB = 262144
# (level, max_chunk_bytes, sizes): every flag, an acceleration, 64 KiB blocks in one and several slots per frame; 256 KiB
# blocks with two slots per frame; 4 MiB blocks whose header ids follow the chunk's size (4, 5, 5)
BATCHES = [(lv, MAXB, R.SIZES) for lv in (0, 4, 0x10, 0x20, 0x40, 0x74, 0x304)] \
    + [(5, 300000, R.SIZES), (7, MAXB, (60000, 70000, 100000))]


def odd_place(parts, extra=()):
    """(host, offs, sizes): the parts at odd byte offsets of one buffer, then the chunks of `extra` ((offset, size) over
    the same buffer: repeated or overlapping chunks)"""
    sizes = [len(p) for p in parts]
    offs, total = layout(sizes, residues=(1, 3))
    host = np.zeros(total, np.uint8)
    for o, p in zip(offs, parts):
        host[o: o + len(p)] = p
    offs = np.concatenate([offs, np.array([e[0] for e in extra], np.int64)])
    return host, offs, sizes + [e[1] for e in extra]


def decode_back(torch, rc, host, offs, sizes, skip=(), **kw):
    """rc's last batch decoded to slices at odd offsets of a fresh canvas with canaries between them"""
    out_offs, total = layout(sizes, residues=(3, 1), gap=7)
    canvas = np.full(total, 0xEE, np.uint8)
    for o, so, s in zip(out_offs, offs, sizes):
        canvas[o: o + s] = host[so: so + s]
    out = torch.full((total,), 0xEE, dtype=torch.uint8, device="cuda")
    rc.decompress(out, out_offs, sizes, **kw)
    torch.cuda.synchronize()
    st = rc.status[: len(sizes)].cpu().numpy()
    assert_roundtrip(st, out.cpu().numpy(), canvas, out_offs, sizes, skip)
    return st


@pytest.fixture(scope="module")
def parts():
    return {sizes: R.batch_parts(sizes) for sizes in {b[2] for b in BATCHES}}


@pytest.mark.parametrize("level,maxb,sizes", BATCHES, ids=[f"{b[0]:#x}-{b[1]}-{len(b[2])}" for b in BATCHES])
def test_frames_are_the_oracles_and_decode_back(torch_cuda, parts, level, maxb, sizes):
    torch = torch_cuda
    p = parts[sizes]
    base_offs, _ = layout([len(x) for x in p], residues=(1, 3))
    big = int(np.argmax(sizes))
    # one chunk twice, and one chunk that starts inside another and runs past a block boundary of it
    extra = [(int(base_offs[1]), sizes[1]), (int(base_offs[big]) + 1001, min(65537, sizes[big] - 1001))]
    host, offs, szs = odd_place(p, extra)
    assert all(o % 2 for o in offs[:len(p)])
    rc = L.RaggedCodec("lz4frame", maxb, len(szs), level=level)
    rc.compress(to_dev(torch, host), offs, szs)
    cs, of, packed = check_batch(torch, rc, len(szs), lambda i: R.stored(host[offs[i]: offs[i] + szs[i]], level))
    if 0 in szs:
        assert cs[szs.index(0)] == (15 if level & 0x20 else 11)
    if level == 7:     # LZ4F_optimalBSID: the id of the smallest block size that holds the chunk
        assert [int(packed[of[i] + 5]) >> 4 for i in range(3)] == [4, 5, 5]
    st = decode_back(torch, rc, host, offs, szs)                       # d_offsets given
    if 0 in szs:
        assert st[szs.index(0)] == 0                                   # the empty frame
    decode_back(torch, rc, host, offs, szs, csizes=rc.csizes)          # d_offsets NULL: scanned into temp


@pytest.mark.parametrize("level", [4, 0x74])
def test_equal_chunks_over_contiguous_input_are_the_uniform_call(torch_cuda, level):
    torch = torch_cuda
    part, k = 100000, 5
    data = L.datagen("mixed", part * k, seed=31)
    d_in = to_dev(torch, data, 256)
    dc = L.DeviceCodec("lz4frame", part * k, part, level=level)
    dc.compress(d_in)
    rc = L.RaggedCodec("lz4frame", part, k, level=level)
    rc.compress(d_in, np.arange(k) * part, [part] * k)
    torch.cuda.synchronize()
    assert (rc.csizes[:k].cpu().numpy() == dc.csizes[:k].cpu().numpy()).all()
    assert (rc.offsets[: k + 1].cpu().numpy() == dc.offsets[: k + 1].cpu().numpy()).all()
    total = dc.packed_total()
    assert total == rc.packed_total() and (rc.packed[:total].cpu().numpy() == dc.packed[:total].cpu().numpy()).all()


def test_a_chunk_over_max_chunk_bytes_is_not_processed(torch_cuda):
    torch = torch_cuda
    sizes = [4096, 70001, 70000, 0, 65537]
    over = {1}
    host, offs, sizes = place([L.datagen("text", n, seed=50 + i) for i, n in enumerate(sizes)])
    rc = L.RaggedCodec("lz4frame", 70000, len(sizes), level=0x74, max_total_bytes=sum(sizes))
    rc.packed.fill_(0xA5)
    rc.compress(to_dev(torch, host), offs, sizes)
    cs, of, _ = check_batch(torch, rc, len(sizes), lambda i: R.stored(host[offs[i]: offs[i] + sizes[i]], 0x74), skip=over)
    assert cs[1] == 0 and of[2] == of[1]                    # no packed bytes
    assert (rc.packed[int(of[-1]):].cpu().numpy() == 0xA5).all()
    st = decode_back(torch, rc, host, offs, sizes, skip=over)         # nothing written for it either
    assert st[1] == -1


def test_packed_cap_is_enforced_on_the_device(torch_cuda):
    torch = torch_cuda
    sizes = [30000, 0, 140000, 65536, 13, 70000]
    kinds = ["text", "text", "mixed", "random", "text", "json"]
    host, offs, sizes = place([L.datagen(k, n, seed=60 + i) for i, (k, n) in enumerate(zip(kinds, sizes))])
    k = len(sizes)
    exp = [R.stored(host[offs[i]: offs[i] + sizes[i]], 0x60) for i in range(k)]
    ends = np.cumsum([len(e) for e in exp])
    cap = int(ends[2]) + 5                                  # frames 0 .. 2 fit, frame 3 would pass the cap, 4 and 5 start past it
    rc = L.RaggedCodec("lz4frame", 140000, k, level=0x60)
    rc.packed.fill_(0xA5)
    d, _ = rc._arrays(to_dev(torch, host), offs, sizes, 16)
    rc._in, rc.k = d, k
    rc._call(rc._crec, in_ptrs=d[0].data_ptr(), in_bytes=d[1].data_ptr(), packed=rc.packed.data_ptr(), packed_cap=cap,
             csizes=rc.csizes.data_ptr(), offsets=rc.offsets.data_ptr(), temp=rc.ctemp.data_ptr(),
             temp_bytes=rc.ctemp.numel())
    torch.cuda.synchronize()
    cs = rc.csizes[:k].cpu().numpy()
    of = rc.offsets[: k + 1].cpu().numpy()
    assert (cs == [len(e) for e in exp]).all() and (of[1:] == ends).all()     # every size is still reported
    assert of[k] > cap
    packed = rc.packed.cpu().numpy()
    assert packed[: ends[2]].tobytes() == b"".join(exp[:3])
    assert (packed[ends[2]:] == 0xA5).all()                 # the frames that do not fit are unwritten: the canary stays


@pytest.mark.parametrize("level", [0x80, 0x84, 0xB0])
def test_decodes_the_oracles_frames_linked_blocks_too(torch_cuda, level):
    torch = torch_cuda
    sizes = [65537, 200000, (1 << 20) + 17]
    parts = [L.datagen("mixed", n, seed=70 + i) for i, n in enumerate(sizes)]
    frames = [R.frame(p, level) for p in parts]
    assert all((f[4] >> 5) & 1 == 0 for f in frames), "the oracle wrote linked frames"
    rc = L.RaggedCodec("lz4frame", 2 << 20, len(sizes))
    st, out, offs = decode_frames(torch, rc, frames, sizes)
    assert st.tolist() == sizes
    canvas = np.full(len(out), 0xEE, np.uint8)
    for o, p in zip(offs, parts):
        canvas[o: o + len(p)] = p
    assert (out == canvas).all()


def test_corrupted_frames_get_the_oracles_verdicts(torch_cuda):
    torch = torch_cuda
    n = R.VERDICT_SIZE
    data, frames = R.corrupted_frames()
    assert len(frames) == R.VERDICT_FRAMES == 200
    rc = L.RaggedCodec("lz4frame", n, 50)
    dc = L.DeviceCodec("lz4frame", 50 * n, n)
    skipped = 0
    for b0 in range(0, len(frames), 50):
        batch = [s for s, _ in frames[b0: b0 + 50]]
        st, out, offs = decode_frames(torch, rc, batch, [n] * len(batch))
        # the uniform call on the same frames: the ragged call's statuses are its statuses
        dc.decompress(packed=to_dev(torch, np.frombuffer(b"".join(batch), np.uint8), 256),
                      csizes=torch.tensor([len(s) for s in batch], dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        uniform = dc.status[: len(batch)].cpu().numpy()
        assert (st == uniform).all(), (b0, np.nonzero(st != uniform)[0])
        for j, s in enumerate(batch):
            r, want = R.decode(s, n)
            # left out: what the uniform call puts outside the supported set (a frame whose blocks are not all full
            # but the last decodes short in the oracle); a frame of the chunk's own size would read as stored raw
            if uniform[j] == -2 or r == -2 or len(s) == n:
                skipped += 1
                continue
            assert (st[j] >= 0) == (r >= 0), f"frame {b0 + j} (level {frames[b0 + j][1]:#x}): gpu {st[j]} oracle {r}"
            if r >= 0:
                assert st[j] == r and out[offs[j]: offs[j] + n].tobytes() == want.tobytes(), b0 + j
    # (with the oracle alone: 5 of this seed's 200 frames decode short or answer -2)
    assert skipped <= len(frames) // 10, skipped


@pytest.mark.parametrize("delta", [-1, 1])
def test_a_wrong_output_size_is_refused_and_stays_inside(torch_cuda, delta):
    torch = torch_cuda
    n = R.VERDICT_SIZE
    data = L.datagen("text", n, seed=9)
    levels = (0, 0x20, 0x40, 0x70, 0x80, 0xB0)
    frames = [R.frame(data, p) for p in levels]
    rc = L.RaggedCodec("lz4frame", n + 1, len(frames))
    st, out, offs = decode_frames(torch, rc, frames, [n + delta] * len(frames))
    assert (st < 0).all(), st
    inside = np.zeros(len(out), bool)
    for o in offs:
        inside[o: o + n + delta] = True
    assert (out[~inside] == 0xEE).all(), "bytes written past d_out_bytes[i]"


def test_capture_compress_and_decompress_in_a_graph(torch_cuda):
    torch = torch_cuda
    sizes = (0, 13, 4096, 65537, 100000)
    host, offs, sizes = place(R.batch_parts(sizes, seed=80))
    k, level = len(sizes), 0x74
    rc = L.RaggedCodec("lz4frame", 100000, k, level=level)
    buf = to_dev(torch, host)
    out = torch.zeros(len(host), dtype=torch.uint8, device="cuda")
    d_src, _ = rc._arrays(buf, offs, sizes, 16)
    d_dst, _ = rc._arrays(out, offs, sizes, 0)

    def pair():
        rc.compress_arrays(d_src, k)
        rc.decompress_arrays(d_dst, k)

    def check():
        torch.cuda.synchronize()
        _, _, packed = check_batch(torch, rc, k, lambda i: R.stored(host[offs[i]: offs[i] + sizes[i]], level))
        got = out.cpu().numpy()
        assert (rc.status[:k].cpu().numpy() == np.array(sizes)).all()
        for o, s in zip(offs, sizes):
            assert (got[o: o + s] == host[o: o + s]).all()
        return packed.tobytes()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):       # every launch on the one stream: no parallel branches
        pair()
    replays = []
    for _ in range(2):
        for t in (out, rc.packed, rc.csizes, rc.offsets, rc.status):
            t.zero_()
        g.replay()
        replays.append(check())
    assert replays[0] == replays[1]
