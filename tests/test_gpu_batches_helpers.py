"""The two numpy checkers of tests/gpu_batches.py, which every ragged GPU test rests on, and its layout(): each
passes on a correct three-chunk batch and raises on every single mutation of it.  No device."""
import numpy as np
import pytest

from gpu_batches import SLACK, assert_packed, assert_roundtrip, layout

SIZES = [7, 0, 5]                               # one empty chunk
FRAMES = [b"first frame", b"\x00", b"third"]    # what a compressor wrote for them
FILL = 0xEE
ROTATIONS = [(1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2), (0, 1, 2, 3)]


def packed_batch():
    cs = np.array([len(f) for f in FRAMES], np.int64)
    of = np.concatenate([[0], np.cumsum(cs)])
    return cs, of, np.frombuffer(b"".join(FRAMES), np.uint8).copy()


def decoded_batch(residues=(1, 2, 3, 0)):
    """(status, output, host, offs): three chunks take the first three of the residues; ROTATIONS reach all four"""
    offs, total = layout(SIZES, residues)
    assert [int(o) % 4 for o in offs] == list(residues[:3])
    host = np.zeros(total, np.uint8)
    for i, (o, s) in enumerate(zip(offs, SIZES)):
        host[o: o + s] = np.arange(s) + 16 * (i + 1)
    got = np.full(total, FILL, np.uint8)
    for o, s in zip(offs, SIZES):
        got[o: o + s] = host[o: o + s]
    return np.array(SIZES, np.int32), got, host, offs


def test_assert_packed_passes_on_the_correct_batch():
    cs, of, packed = packed_batch()
    assert_packed(cs, of, packed, int(of[3]), FRAMES)
    assert_packed(cs, of, packed, int(of[3]), lambda i: FRAMES[i])


@pytest.mark.parametrize("entry", [0, 1, 2, 3])
def test_assert_packed_one_offset_off_by_one(entry):
    cs, of, packed = packed_batch()
    of[entry] += 1
    with pytest.raises(AssertionError, match="exclusive scan"):
        assert_packed(cs, of, packed, int(cs.sum()), FRAMES)


@pytest.mark.parametrize("delta", [-1, 1])
def test_assert_packed_total_off_by_one(delta):
    cs, of, packed = packed_batch()
    with pytest.raises(AssertionError):
        assert_packed(cs, of, packed, int(of[3]) + delta, FRAMES)


def test_assert_packed_one_csize_wrong():
    """a size that disagrees with the expected frame, the offsets and the total consistent with it"""
    cs, of, packed = packed_batch()
    cs[2] -= 1
    of = np.concatenate([[0], np.cumsum(cs)])
    with pytest.raises(AssertionError, match="chunk 2: csize 4, expected 5"):
        assert_packed(cs, of, packed[:-1], int(of[3]), FRAMES)


@pytest.mark.parametrize("chunk", [0, 1, 2])
def test_assert_packed_one_byte_flipped(chunk):
    cs, of, packed = packed_batch()
    packed[of[chunk + 1] - 1] ^= 0x01
    with pytest.raises(AssertionError, match=f"chunk {chunk}: packed bytes differ"):
        assert_packed(cs, of, packed, int(of[3]), FRAMES)
    assert_packed(cs, of, packed, int(of[3]), FRAMES, skip={chunk})      # a skipped chunk's bytes are not compared


def test_assert_packed_does_not_ask_for_a_skipped_chunk():
    cs, of, packed = packed_batch()

    def expected(i):
        assert i != 1
        return FRAMES[i]

    assert_packed(cs, of, packed, int(of[3]), expected, skip={1})


@pytest.mark.parametrize("residues", ROTATIONS)
def test_assert_roundtrip_passes_on_the_correct_batch(residues):
    st, got, host, offs = decoded_batch(residues)
    assert_roundtrip(st, got, host, offs, SIZES)
    assert_roundtrip(st, got, host, offs, SIZES, fill=FILL)


@pytest.mark.parametrize("chunk", [0, 1, 2])
def test_assert_roundtrip_one_status_wrong(chunk):
    st, got, host, offs = decoded_batch()
    st[chunk] = -1
    with pytest.raises(AssertionError, match=f"chunk {chunk}: status -1"):
        assert_roundtrip(st, got, host, offs, SIZES)


@pytest.mark.parametrize("chunk,at", [(0, 0), (0, 6), (2, 0), (2, 4)])
def test_assert_roundtrip_one_byte_inside_a_chunk_flipped(chunk, at):
    st, got, host, offs = decoded_batch()
    got[offs[chunk] + at] ^= 0x80
    with pytest.raises(AssertionError, match=f"chunk {chunk}: roundtrip"):
        assert_roundtrip(st, got, host, offs, SIZES)


@pytest.mark.parametrize("chunk", [0, 1, 2])
@pytest.mark.parametrize("side", ["before", "after"])
@pytest.mark.parametrize("residues", ROTATIONS)
def test_assert_roundtrip_a_gap_byte_next_to_a_chunk_is_not_the_fill(residues, chunk, side):
    st, got, host, offs = decoded_batch(residues)
    got[offs[chunk] - 1 if side == "before" else offs[chunk] + SIZES[chunk]] = 0
    with pytest.raises(AssertionError, match="wrote outside the chunks"):
        assert_roundtrip(st, got, host, offs, SIZES)


def test_assert_roundtrip_other_fill():
    st, got, host, offs = decoded_batch()
    with pytest.raises(AssertionError, match="wrote outside the chunks"):
        assert_roundtrip(st, got, host, offs, SIZES, fill=0xA5)


def test_assert_roundtrip_a_skipped_chunk_counts_as_outside():
    """a skipped chunk (an oversize one: status -1, nothing written) is not compared, and a write into its range
    raises"""
    st, got, host, offs = decoded_batch()
    st[0] = -1
    got[offs[0]: offs[0] + SIZES[0]] = FILL
    assert_roundtrip(st, got, host, offs, SIZES, skip={0})
    got[offs[0] + 3] = host[offs[0] + 3]
    with pytest.raises(AssertionError, match="wrote outside the chunks"):
        assert_roundtrip(st, got, host, offs, SIZES, skip={0})


@pytest.mark.parametrize("sizes,residues,gap", [([7, 0, 5, 1, 4099, 0, 0, 2, 65536], (1, 2, 3, 0), 5),
                                                 ([3, 3, 3, 3, 3], (0, 2), 1), ([0, 0, 0], (3,), 9)])
def test_layout(sizes, residues, gap):
    offs, total = layout(sizes, residues, gap)
    assert len(offs) == len(sizes) and offs.dtype == np.int64
    ends = [0] + [int(o) + s for o, s in zip(offs, sizes)]
    for i, o in enumerate(offs):
        assert o - ends[i] >= gap                  # a gap before every chunk, so the offsets strictly increase
        assert o % 4 == residues[i % len(residues)]
    assert (np.diff(offs) > 0).all()
    assert total == ends[-1] + SLACK


def test_layout_defaults():
    offs, total = layout(SIZES)
    assert [int(o) % 4 for o in layout([1] * 8)[0]] == [1, 2, 3, 0] * 2
    assert int(offs[0]) >= 5 and total == int(offs[2]) + SIZES[2] + SLACK
