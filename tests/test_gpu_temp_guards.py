"""GPU: the temp buffers of the uniform device API (lzh_compress_async / lzh_decompress_async, all six codecs) and of
the ragged decode at exactly their sizing answer, between guard bytes: nothing is written outside them, the round
trip gives the input back, and the packed bytes are the CPU oracle's.  Run with -m gpu."""
import numpy as np
import pytest

import oracle_lib as O
import lzbench_amd as L
from gpu_batches import check_batch, to_dev, torch_cuda
from ragged_inputs import EDGE_SIZES, edge_input, expected

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0xEE
BIG = (16 << 20) + 4096      # above the parse + emit split's largest chunk: the single-kernel path, no record area

# (codec name, level, oracle codec or None (memcpy: the input), chunk, n, corpus)
CASES = []
for _name, _lvl in (("lz4", 1), ("lz4fast", 7), ("snappy", 0)):
    CASES.append((_name, _lvl, _name, 4096, 5 * 4096 + 17, "mixed"))        # one snappy fragment, short last chunk
    CASES.append((_name, _lvl, _name, 100000, 3 * 100000 + 1, "mixed"))     # two snappy fragments: split decoder's temp
for _name, _lvl in (("lz4", 1), ("snappy", 0)):
    CASES.append((_name, _lvl, _name, BIG, BIG + 5, "text"))
for _lvl in (1, -1):
    CASES.append(("zstd", _lvl, "zstd", 4096, 3 * 4096 + 17, "mixed"))      # below lzh_zstd_split_min: one-wave decoder
    CASES.append(("zstd", _lvl, "zstd", 65536, 3 * 65536 + 17, "mixed"))    # split decoder, scratch per frame
CASES.append(("lz4frame", 4, "lz4f", 200000, 2 * 200000 + 9, "mixed"))     # 64 KiB blocks, 4 blocks per frame
CASES.append(("lz4frame", 4 | L.LZ4F_LINKED, "lz4f", 200000, 2 * 200000 + 9, "mixed"))
CASES.append(("nvcomp_lz4", 0, "nvlz4", 100000, 2 * 100000 + 9, "mixed"))
CASES.append(("memcpy", 0, None, 4096, 10000, "mixed"))
IDS = [f"{c[0]}{c[1]:#x}-b{c[3]}" if c[0] == "lz4frame" else f"{c[0]}{c[1]}-b{c[3]}" for c in CASES]


def guarded(torch, nbytes):
    """nbytes of device memory between two guards of GUARD bytes (the slice keeps the allocation's alignment)."""
    buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return buf[GUARD: GUARD + nbytes], (buf[:GUARD], buf[GUARD + nbytes:])


def intact(torch, guards):
    torch.cuda.synchronize()
    return all(bool((g == FILL).all()) for g in guards)


@pytest.mark.parametrize("name,level,oracle,chunk,n,corpus", CASES, ids=IDS)
def test_uniform_temp_at_the_sizing_answer(torch_cuda, name, level, oracle, chunk, n, corpus):
    torch = torch_cuda
    lib = L.lib()
    host = L.datagen(corpus, n, seed=61)
    d_in = to_dev(torch, host, 64)
    dc = L.DeviceCodec(name, n, chunk, level)
    dc.ctemp, cguards = guarded(torch, lib.lzh_compress_temp_bytes(dc.codec, n, chunk))
    dc.dtemp, dguards = guarded(torch, lib.lzh_decompress_temp_bytes(dc.codec, n, chunk))
    dc.compress(d_in)
    assert intact(torch, cguards), "compress wrote outside its temp"
    k = dc.k
    part = np.minimum(chunk, n - np.arange(k) * chunk)
    cs = dc.csizes.cpu().numpy().astype(np.uint64)
    of = dc.offsets.cpu().numpy().astype(np.uint64)
    assert (of == np.concatenate([[0], np.cumsum(cs)])).all(), "offsets are not the exclusive scan of csizes"
    packed = dc.packed[: dc.packed_total()].cpu().numpy()
    if oracle is None:
        exp, ecs = host, part.astype(np.uint64)
    else:
        exp, ecs = O.compress_chunks(host, oracle, chunk, level, use_ref=False)
    assert (cs == ecs).all(), "chunk sizes differ from the oracle's"
    assert len(packed) == len(exp) and (packed == exp).all(), "packed bytes differ from the oracle's"
    # decode with the compressor's offsets, then with offsets derived on the device (the scan lands in temp)
    for offsets in (dc.offsets, None):
        dc.out.zero_()
        dc.status.fill_(-7)
        dc.decompress(offsets=offsets)
        assert intact(torch, dguards), f"decompress wrote outside its temp (offsets {'given' if offsets is not None else 'None'})"
        assert (dc.status.cpu().numpy() == part).all()
        assert (dc.out[:n].cpu().numpy() == host).all(), "round trip"
    assert intact(torch, cguards)


@pytest.mark.parametrize("codec,level", [("lz4", 1), ("snappy", 0)], ids=["lz4", "snappy"])
def test_ragged_decode_temp_at_the_sizing_answer(torch_cuda, edge_input, codec, level):
    torch = torch_cuda
    host, offs = edge_input
    k, maxb = len(EDGE_SIZES), max(EDGE_SIZES)
    rc = L.RaggedCodec(codec, maxb, k, level, max_total_bytes=sum(EDGE_SIZES))
    rc.dtemp, guards = guarded(torch, L.lib().lzh_ragged_decompress_temp_bytes(rc.codec, maxb, k))
    rc.compress(to_dev(torch, host), offs, EDGE_SIZES)
    check_batch(torch, rc, len(EDGE_SIZES), expected(host, offs, EDGE_SIZES, codec, level))
    for kw in ({}, {"csizes": rc.csizes}):       # the compressor's offsets; offsets=None: scanned into temp
        out = torch.full((len(host),), FILL, dtype=torch.uint8, device="cuda")
        rc.status.fill_(-7)
        rc.decompress(out, offs, EDGE_SIZES, **kw)
        assert intact(torch, guards), "ragged decompress wrote outside its temp"
        assert (rc.status[:k].cpu().numpy() == np.array(EDGE_SIZES)).all()
        got = out.cpu().numpy()
        mask = np.zeros(len(host), bool)
        for o, s in zip(offs, EDGE_SIZES):
            assert (got[o: o + s] == host[o: o + s]).all()
            mask[o: o + s] = True
        assert (got[~mask] == FILL).all(), "the decoder wrote outside the chunks"
