"""GPU decoder fuzz: corrupted LZ4 / snappy streams through the HIP decoders, each verdict and
output checked against the REFERENCE decoders (LZ4_decompress_safe, snappy::RawUncompress,
compiled from /root/reference into oracle/_ref by oracle/Makefile).  A corrupt stream must be
rejected exactly when the reference rejects it, decode to the same bytes when it does not, and
never fault the GPU.  Run with -m gpu."""
import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
from gpu_batches import torch_cuda

pytestmark = pytest.mark.gpu

CAP = 65536
N_STREAMS = 1024


@pytest.fixture(scope="module")
def torch_cuda_ref(torch_cuda):
    """torch_cuda where the reference decoders are present: they are this file's checker"""
    if not O.have_ref():
        pytest.skip("reference build (oracle/_ref) not present")
    return torch_cuda


def _corrupt(rng, s: bytes) -> bytes:
    b = bytearray(s)
    kind = int(rng.integers(0, 5))
    if kind == 0:                                   # a few bytes replaced
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
    elif kind == 1:                                 # one bit flipped in the first 64 bytes
        i = int(rng.integers(0, min(64, len(b))))
        b[i] ^= 1 << int(rng.integers(0, 8))
    elif kind == 2:                                 # truncated
        b = b[: int(rng.integers(1, len(b)))]
    elif kind == 3:                                 # garbage appended
        b += bytes(rng.integers(0, 256, int(rng.integers(1, 64))).astype(np.uint8))
    else:                                           # garbage
        b = bytearray(rng.integers(0, 256, int(rng.integers(1, 2048))).astype(np.uint8).tobytes())
    return bytes(b)


def _varint(s: bytes):
    v, sh = 0, 0
    for i, c in enumerate(s[:5]):
        v |= (c & 0x7F) << sh
        if c < 128:
            return v
        sh += 7
    return None


def _ref_verdict(codec, s: bytes):
    """(size or -1, output bytes) from the reference decoder with capacity CAP."""
    R = O.ref()
    src = np.frombuffer(s, np.uint8).copy()
    if codec == "lz4":
        dst = np.zeros(CAP + 64, np.uint8)
        r = R.ref_lz4_decompress_safe(src.ctypes.data, dst.ctypes.data, len(s), CAP)
        return (r, dst[:r].tobytes()) if r >= 0 else (-1, b"")
    ulen = _varint(s)
    if ulen is None or ulen > CAP:
        return -1, b""
    dst = np.zeros(ulen + 64, np.uint8)
    ok = R.ref_snappy_uncompress(src.ctypes.data, len(s), dst.ctypes.data)
    return (ulen, dst[:ulen].tobytes()) if ok else (-1, b"")


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
@pytest.mark.parametrize("corpus", ["text", "json"])
def test_corrupt_streams_match_reference_verdicts(torch_cuda_ref, codec, corpus):
    torch = torch_cuda_ref
    rng = np.random.default_rng(7 + len(codec) + len(corpus))
    data = L.datagen(corpus, 8 * CAP, seed=99)
    packed, cs = O.compress_chunks(data, codec, CAP)
    offs = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
    valid = [packed[offs[i]:offs[i + 1]].tobytes() for i in range(len(cs))]
    streams = []
    while len(streams) < N_STREAMS:
        s = _corrupt(rng, valid[int(rng.integers(0, len(valid)))])
        if 0 < len(s) != CAP:                       # (clen == part would mean "stored raw")
            streams.append(s)
    blob = b"".join(streams)
    k = len(streams)
    d_packed = torch.zeros(len(blob) + 256, dtype=torch.uint8, device="cuda")
    d_packed[: len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
    d_cs = torch.tensor([len(s) for s in streams], dtype=torch.int32, device="cuda")
    dc = L.DeviceCodec(codec, k * CAP, CAP)
    dc.decompress(packed=d_packed, csizes=d_cs)
    torch.cuda.synchronize()
    status = dc.status[:k].cpu().numpy()
    out = dc.out[: k * CAP].cpu().numpy()
    for i, s in enumerate(streams):
        r, ref_out = _ref_verdict(codec, s)
        st = int(status[i])
        assert (st >= 0) == (r >= 0), f"stream {i}: gpu {st} reference {r}"
        if r >= 0:
            assert st == r, f"stream {i}: gpu size {st} reference {r}"
            assert out[i * CAP: i * CAP + r].tobytes() == ref_out, f"stream {i}: bytes differ"
