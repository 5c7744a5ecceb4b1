"""tests/zstd_hand_frames.py -- valid zstd frames (RFC 8878) built by hand for the branches of the format that no
encoder at hand writes: an RLE block between other blocks, RLE literals at each of the three header sizes (5-,
12- and 20-bit regenerated size) followed by sequences, and a compressed block with no literals whose one
sequence copies from the block before it.  In the style of _rle_seq_frame (tests/test_gpu_zstd.py): the three
sequence tables are RLE-coded (one code each, zero state bits), so a sequence is just its extra bits, and the
expected output follows from the sequences in a few lines (execute()).  Pure Python; the reference build, where
present, must accept every frame and give the same bytes (tests/test_zstd_census.py)."""

# (base, extra bits) of the literal-length, match-length codes (RFC 8878 3.1.1.3.2.1.1); offset code c: (1 << c) + c bits
LL = {c: (c, 0) for c in range(16)}
LL.update({16: (16, 1), 17: (18, 1), 18: (20, 1), 19: (22, 1), 20: (24, 2), 21: (28, 2), 22: (32, 3), 23: (40, 3),
           24: (48, 4), 25: (64, 6), 26: (128, 7), 27: (256, 8), 28: (512, 9), 29: (1024, 10), 30: (2048, 11),
           31: (4096, 12), 32: (8192, 13), 33: (16384, 14), 34: (32768, 15), 35: (65536, 16)})
ML = {c: (c + 3, 0) for c in range(32)}
ML.update({32: (35, 1), 33: (37, 1), 34: (39, 1), 35: (41, 1), 36: (43, 2), 37: (47, 2), 38: (51, 3), 39: (59, 3),
           40: (67, 4), 41: (83, 4), 42: (99, 5), 43: (131, 7), 44: (259, 8), 45: (515, 9), 46: (1027, 10),
           47: (2051, 11), 48: (4099, 12), 49: (8195, 13), 50: (16387, 14), 51: (32771, 15), 52: (65539, 16)})

PATTERN = bytes((37 * i + 11) & 0xFF for i in range(128))      # the raw block ahead of every compressed block


def frame_header(n: int) -> bytes:
    return b"\x28\xb5\x2f\xfd" + bytes([0x20 | (2 << 6)]) + n.to_bytes(4, "little")   # single segment, 4-byte size


def block(btype: int, size: int, body: bytes, last: bool) -> bytes:
    return (int(last) | (btype << 1) | (size << 3)).to_bytes(3, "little") + body


def literals_header(kind: int, regen: int, hdr: int) -> bytes:
    """raw (kind 0) or RLE (kind 1) literals header of `hdr` bytes"""
    if hdr == 1:
        assert regen < 32
        return bytes([kind | (regen << 3)])
    if hdr == 2:
        assert regen < 4096
        return (kind | (1 << 2) | (regen << 4)).to_bytes(2, "little")
    assert regen < (1 << 20)
    return (kind | (3 << 2) | (regen << 4)).to_bytes(3, "little")


def sequences(ll_code: int, of_code: int, ml_code: int, extras) -> bytes:
    """A sequences section with RLE tables for the three codes; extras: per sequence (LL, OF, ML) extra-bit
    values.  The bitstream is read backwards: the first sequence's offset bits come first, then its match-length
    and its literal-length bits (RFC 8878 3.1.1.3.2.1.2)."""
    nseq = len(extras)
    assert 0 < nseq < 128
    llb, ofb, mlb = LL[ll_code][1], of_code, ML[ml_code][1]
    acc, pos = 0, 0
    for ll, of, ml in reversed(extras):
        for v, nb in ((ll, llb), (ml, mlb), (of, ofb)):
            assert 0 <= v < (1 << nb) or (nb == 0 and v == 0)
            acc |= v << pos
            pos += nb
    acc |= 1 << pos                                          # the end mark
    bits = acc.to_bytes(pos // 8 + 1, "little")
    return bytes([nseq, (1 << 6) | (1 << 4) | (1 << 2), ll_code, of_code, ml_code]) + bits


def execute(history: bytes, literals: bytes, ll_code, of_code, ml_code, extras) -> bytes:
    """the bytes a block decodes to after `history`; offsets here are real ones (offset value above 3)"""
    out = bytearray(history)
    lp = 0
    for ll, of, ml in extras:
        n_ll, n_ml = LL[ll_code][0] + ll, ML[ml_code][0] + ml
        offset = (1 << of_code) + of - 3
        assert of_code >= 2 and 0 < offset <= len(out) + n_ll
        out += literals[lp: lp + n_ll]
        lp += n_ll
        for _ in range(n_ml):
            out.append(out[-offset])
    assert lp <= len(literals)
    out += literals[lp:]
    return bytes(out[len(history):])


def rle_block_frame(two: bool = False):
    """raw block, RLE block of 100000 bytes, raw block, RLE block of one byte (the last): more blocks than the
    split decoder's layout holds for a chunk of this size; two: only an RLE block and a raw one, which it holds"""
    parts = [(0, PATTERN), (1, b"\x5a" * 100000), (0, b"tail"), (1, b"\xc3")]
    if two:
        parts = parts[1:3]
    content = b"".join(p for _, p in parts)
    f = frame_header(len(content))
    for i, (t, p) in enumerate(parts):
        f += block(t, len(p), p if t == 0 else p[:1], i == len(parts) - 1)
    return f, content


def _seq_frame(lit_kind, lit_byte, regen, hdr, codes, extras):
    lits = bytes([lit_byte]) * regen
    body = literals_header(lit_kind, regen, hdr) + (lits if lit_kind == 0 else lits[:1])
    body += sequences(*codes, extras)
    content = PATTERN + execute(PATTERN, lits, *codes, extras)
    f = frame_header(len(content)) + block(0, len(PATTERN), PATTERN, False) + block(2, len(body), body, True)
    return f, content


def rle_literals_frame(hdr: int):
    """raw block, then a compressed block of RLE literals (header of `hdr` bytes) and sequences that copy from the
    raw block and from earlier output at varying offsets"""
    if hdr == 1:      # 31 literals; LL 5, offsets 16 + 0..15 - 3, ML 35 + 0..1
        return _seq_frame(1, 0x41, 31, 1, (5, 4, 32), [(0, 9, 1), (0, 0, 0), (0, 15, 1)])
    if hdr == 2:      # 2000 literals; LL 16 + 0..1, offsets 64 + 0..63 - 3, ML 67 + 0..15
        return _seq_frame(1, 0x42, 2000, 2, (16, 6, 40), [(1, 60, 3), (0, 0, 15), (1, 33, 0), (0, 63, 7), (1, 5, 9)])
    # 70000 literals; LL 4096 + 0..4095, offsets 4096 + 0..4095 - 3, ML 259 + 0..255
    return _seq_frame(1, 0x43, 70000, 3, (31, 12, 44), [(4095, 4000, 255), (0, 130, 0), (1234, 77, 200), (17, 4095, 3)])


def no_literals_frame():
    """raw block, then a compressed block whose literals section is empty (raw, size 0) and whose one sequence --
    literal length 0, offset 64 + 40 - 3 = 101, match length 67 + 11 -- copies from the raw block"""
    return _seq_frame(0, 0, 0, 1, (0, 6, 40), [(0, 40, 11)])


def hand_frames():
    """[(name, frame, content)]"""
    out = [("rle_block", *rle_block_frame()), ("rle_block_two", *rle_block_frame(True))]
    out += [(f"rle_literals_hdr{h}", *rle_literals_frame(h)) for h in (1, 2, 3)]
    out.append(("no_literals", *no_literals_frame()))
    return out
