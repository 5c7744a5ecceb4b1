"""What the GPU tests of the dictionary calls (test_gpu_lz4_dict.py, test_gpu_zstd_dict.py and, through the latter,
test_gpu_zstd_dfast_dict.py) share to lay a ragged batch out in one flat buffer, move it to the device and check the
round trip.  A plain module: no fixtures, no tests."""
import numpy as np

SLACK = 64


def layout(sizes, gap=5):
    """Offsets for chunks of `sizes` in one flat buffer: gaps between chunks, pointers over all residues mod 4."""
    offs, pos = [], 0
    for i, s in enumerate(sizes):
        pos += gap
        pos += ((1, 2, 3, 0)[i % 4] - pos) % 4
        offs.append(pos)
        pos += s
    return np.array(offs, np.int64), pos + SLACK


def to_dev(torch, a: np.ndarray, pad=0):
    t = torch.zeros(len(a) + pad, dtype=torch.uint8, device="cuda")
    t[: len(a)].copy_(torch.from_numpy(np.array(a, np.uint8)))
    return t


def roundtrip(torch, rc, host, offs, sizes, skip=(), **kw):
    out = torch.full((len(host),), 0xEE, dtype=torch.uint8, device="cuda")
    rc.decompress(out, offs, sizes, **kw)
    torch.cuda.synchronize()
    st = rc.status[: len(sizes)].cpu().numpy()
    got = out.cpu().numpy()
    mask = np.zeros(len(host), bool)
    for i in range(len(sizes)):
        if i in skip:
            continue
        assert int(st[i]) == sizes[i], f"chunk {i}: status {st[i]}"
        assert (got[offs[i]: offs[i] + sizes[i]] == host[offs[i]: offs[i] + sizes[i]]).all(), f"chunk {i}: roundtrip"
        mask[offs[i]: offs[i] + sizes[i]] = True
    assert (got[~mask] == 0xEE).all(), "the decoder wrote outside the chunks"
    return st
