"""GPU: lzh_compress_kernel_stage in parts.  For the codecs whose compression is two kernels -- LZ4 and snappy on the
split path, LZ4 frames with independent blocks -- stage_mask 1 (parse) and then stage_mask 2 (emit; frames: and the
frame sizes) leave the sizes and the staging slots that one call with stage_mask 3 leaves, and the pack that follows
(lzh_compress_finish_async; frames have none of their own: lzh_compress_async on the same buffers) gives the packed
bytes of a plain lzh_compress_async."""
import numpy as np
import pytest

import lzbench_amd as L
from gpu_batches import to_dev, torch_cuda

# (codec, n, chunk_size): a one-byte tail chunk; a one-byte input; snappy chunks of two fragments, the last chunk short
SHAPES = [(c, n, 4096) for c in ("lz4", "snappy", "lz4frame") for n in (3 * 4096 + 1, 1)] + [("snappy", 131072 + 70000, 131072)]


def fresh(torch, codec, n, chunk):
    dc = L.DeviceCodec(codec, n, chunk)
    for t in (dc.ctemp, dc.packed, dc.csizes, dc.offsets):
        t.zero_()
    return dc


def staged(dc, codec, n, chunk):
    """The staging bytes the pack reads: slot i (the slots come first in the temp) up to the chunk's compressed size,
    for the chunks that are not stored raw -- past that a slot holds whatever the emit kernel's wide stores left.
    A frame of up to 64 KiB is one block, compressed as an LZ4 chunk; with level 0 its frame is a 7-byte header, the
    block's 4-byte word, the block and the 4-byte end mark."""
    lz4f = codec == "lz4frame"
    stride = L.lib().lzh_stage_stride(L.CODECS["lz4"] if lz4f else dc.codec, chunk)
    temp = dc.ctemp[: dc.k * stride].cpu().numpy()
    cs = dc.csizes.cpu().numpy().astype(np.int64) - (15 if lz4f else 0)
    raw = [min(chunk, n - i * chunk) for i in range(dc.k)]
    return [temp[i * stride: i * stride + cs[i]].tobytes() for i in range(dc.k) if cs[i] < raw[i]]


def packed(torch, dc):
    torch.cuda.synchronize()
    of = dc.offsets.cpu().numpy()
    cs = dc.csizes.cpu().numpy().astype(np.int64)
    assert (of == np.concatenate([[0], np.cumsum(cs)])).all()
    return cs, dc.packed[: int(of[dc.k])].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("codec,n,chunk", SHAPES, ids=lambda v: str(v))
def test_stages_one_by_one_equal_the_whole(torch_cuda, codec, n, chunk):
    torch = torch_cuda
    d_in = to_dev(torch, L.datagen("text", n, seed=n), 256)
    parts, whole, plain = (fresh(torch, codec, n, chunk) for _ in range(3))
    parts.compress_stage(d_in, 1)
    parts.compress_stage(d_in, 2)
    whole.compress_stage(d_in, 3)
    plain.compress(d_in)
    torch.cuda.synchronize()
    cs = whole.csizes.cpu().numpy()
    assert (cs > 0).all() and (parts.csizes.cpu().numpy() == cs).all()
    slots = staged(whole, codec, n, chunk)
    assert staged(parts, codec, n, chunk) == slots and len(slots) == whole.k - (n % chunk == 1)   # (1 byte: raw)
    want_cs, want = packed(torch, plain)
    assert (want_cs == cs).all()
    if codec == "lz4frame":
        parts.compress(d_in)
    else:
        parts.compress_finish(d_in)
    got_cs, got = packed(torch, parts)
    assert (got_cs == want_cs).all() and got.tobytes() == want.tobytes()
