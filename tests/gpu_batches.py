"""What the GPU tests share: the device fixture, the flat layout of a ragged batch, the move to the device, and the
checks every ragged test rests on (the offsets are a scan, the packed bytes are the expected ones, the decoder wrote
nothing outside the chunks).  A plain module: no tests.  assert_packed and assert_roundtrip are numpy alone and have
tests of their own (tests/test_gpu_batches_helpers.py)."""
import hashlib

import numpy as np
import pytest

SLACK = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    return torch


def layout(sizes, residues=(1, 2, 3, 0), gap=5):
    """Offsets for chunks of `sizes` in one flat buffer: gaps between chunks, pointers over all residues mod 4."""
    offs, pos = [], 0
    for i, s in enumerate(sizes):
        pos += gap
        pos += (residues[i % len(residues)] - pos) % 4
        offs.append(pos)
        pos += s
    return np.array(offs, np.int64), pos + SLACK


def place(parts):
    """(host, offs, sizes): the parts laid out by layout() in one zeroed buffer"""
    sizes = [len(p) for p in parts]
    offs, total = layout(sizes)
    host = np.zeros(total, np.uint8)
    for o, p in zip(offs, parts):
        host[o: o + len(p)] = p
    return host, offs, sizes


def to_dev(torch, a: np.ndarray, pad=0):
    t = torch.zeros(len(a) + pad, dtype=torch.uint8, device="cuda")
    t[: len(a)].copy_(torch.from_numpy(np.array(a, dtype=np.uint8)))   # (a writable copy: frombuffer views are not)
    return t


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def assert_packed(cs, of, packed, packed_total, expected, skip=()):
    """A compress call's csizes, offsets ([k + 1]) and packed bytes against expected: a sequence of bytes, or a
    callable from chunk index to bytes (not called for a chunk in skip)."""
    k = len(cs)
    assert (of == np.concatenate([[0], np.cumsum(cs)])).all(), "offsets are not the exclusive scan of csizes"
    assert packed_total == int(cs.sum())
    for i in range(k):
        if i in skip:
            continue
        e = expected(i) if callable(expected) else expected[i]
        assert int(cs[i]) == len(e), f"chunk {i}: csize {cs[i]}, expected {len(e)}"
        assert packed[of[i]: of[i + 1]].tobytes() == e, f"chunk {i}: packed bytes differ"


def assert_roundtrip(st, got, host, offs, sizes, skip=(), fill=0xEE):
    """A decode call's statuses and its output buffer (filled with `fill` before the call) against host; a chunk in
    skip is not compared and counts as outside."""
    mask = np.zeros(len(host), bool)
    for i in range(len(sizes)):
        if i in skip:
            continue
        assert int(st[i]) == sizes[i], f"chunk {i}: status {st[i]}"
        assert (got[offs[i]: offs[i] + sizes[i]] == host[offs[i]: offs[i] + sizes[i]]).all(), f"chunk {i}: roundtrip"
        mask[offs[i]: offs[i] + sizes[i]] = True
    assert (got[~mask] == fill).all(), "the decoder wrote outside the chunks"


def check_batch(torch, rc, k, expected, skip=()):
    """csizes, offsets and every packed byte range of rc's last compress call (k chunks) against expected."""
    torch.cuda.synchronize()
    cs = rc.csizes[:k].cpu().numpy().astype(np.int64)
    of = rc.offsets[: k + 1].cpu().numpy()
    packed = rc.packed[: int(of[k])].cpu().numpy()
    assert_packed(cs, of, packed, rc.packed_total(), expected, skip)
    return cs, of, packed


def roundtrip(torch, rc, host, offs, sizes, skip=(), **kw):
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    rc.decompress(out, offs, sizes, **kw)
    torch.cuda.synchronize()
    st = rc.status[: len(sizes)].cpu().numpy()
    assert_roundtrip(st, out.cpu().numpy(), host, offs, sizes, skip)
    return st


def decode_frames(torch, rc, frames, out_sizes, **kw):
    """frames (bytes each) as one ragged batch through rc, offsets derived from the sizes on the device:
    (status, output canvas, output offsets)"""
    offs, total = layout(out_sizes)
    out = torch.full((total,), 0xEE, dtype=torch.uint8, device="cuda")
    packed = to_dev(torch, np.frombuffer(b"".join(frames), np.uint8), 256)
    csizes = torch.tensor([len(f) for f in frames], dtype=torch.int32, device="cuda")
    rc.decompress(out, offs, out_sizes, packed=packed, csizes=csizes, **kw)
    torch.cuda.synchronize()
    return rc.status[: len(frames)].cpu().numpy(), out.cpu().numpy(), offs
