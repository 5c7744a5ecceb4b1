"""tests/zstd_census.py -- which branches of the zstd frame format a frame takes (RFC 8878).  Pure Python, no GPU.

walk(frame) goes through one frame -- the frame header (every content-size width, single segment or window
descriptor, dictionary id, optional checksum), each block header, the literals-section header (with the Huffman
tree header's kind) and the sequences-section header -- and counts the classes below; it decodes no entropy
stream.  It must end exactly on the frame's last byte (the 4 checksum bytes included when the flag is set) and
raises CensusError on anything else: a truncated or overlong frame, a reserved block type, a section that does
not fit its block.

  block/{raw,rle,cmp}               per block
  blocks/{1,2+}                     per frame
  lit/{raw,rle}/hdr{1,2,3}          raw and RLE literals by header bytes (5-, 12- and 20-bit regenerated size)
  lit/{huf,treeless}/sf{0..3}       Huffman literals by size format (0: one stream; 1-3: four, 10/14/18-bit sizes)
  hufhdr/{fse,direct}               the tree description of a lit/huf section: FSE-coded or 4-bit weights
  lit/regen=0                       a literals section of no bytes
  nseq/{0,1-127,128-32511,long}     the sequence count by header form (long: the 3-byte form, 0x7F00 and more)
  {LL,OF,ML}/{predef,rle,fse,repeat}  the three table modes of a block with sequences

The long-length escapes are not visible in the headers; they follow from sizes: in a single-block frame of
content size N whose block has one sequence, the match is N - regen_size bytes long and the literals before it
at most regen_size (walk() returns (regen_size, nseq) per compressed block)."""
from collections import Counter

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 1 << 17
MODES = ("predef", "rle", "fse", "repeat")

BLOCK_CLASSES = ["block/raw", "block/rle", "block/cmp", "blocks/1", "blocks/2+"]
LIT_CLASSES = ([f"lit/{t}/hdr{h}" for t in ("raw", "rle") for h in (1, 2, 3)]
               + [f"lit/{t}/sf{s}" for t in ("huf", "treeless") for s in range(4)]
               + ["hufhdr/fse", "hufhdr/direct", "lit/regen=0"])
SEQ_CLASSES = (["nseq/0", "nseq/1-127", "nseq/128-32511", "nseq/long"]
               + [f"{t}/{m}" for t in ("LL", "OF", "ML") for m in MODES])
ALL_CLASSES = BLOCK_CLASSES + LIT_CLASSES + SEQ_CLASSES


class CensusError(ValueError):
    pass


def _need(cond, what):
    if not cond:
        raise CensusError(what)


def frame_header(frame: bytes):
    """(header bytes, content size or None, checksum flag) of a frame (RFC 8878 3.1.1.1)"""
    _need(len(frame) >= 6 and frame[:4] == MAGIC, "no zstd magic")
    fhd = frame[4]
    fcs_flag, single, checksum, did_flag = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
    _need(not fhd & 0x08, "reserved frame-header bit")
    p = 5 + (0 if single else 1)
    p += (0, 1, 2, 4)[did_flag]
    w = (1 if single else 0, 2, 4, 8)[fcs_flag]
    _need(p + w <= len(frame), "frame header past the end")
    fcs = None
    if w:
        fcs = int.from_bytes(frame[p:p + w], "little") + (256 if w == 2 else 0)
    return p + w, fcs, checksum


def _literals(c, b: bytes):
    """the literals section at the head of block content b: (section bytes, regenerated size)"""
    _need(len(b) >= 1, "empty compressed block")
    kind, sf = b[0] & 3, (b[0] >> 2) & 3
    if kind < 2:
        name = ("raw", "rle")[kind]
        hsz = 1 if not sf & 1 else (2 if sf == 1 else 3)
        _need(len(b) >= hsz, "literals header past the block")
        h = int.from_bytes(b[:hsz], "little")
        regen = h >> 3 if hsz == 1 else h >> 4
        c[f"lit/{name}/hdr{hsz}"] += 1
        size = hsz + (regen if kind == 0 else 1)
    else:
        name = ("huf", "treeless")[kind - 2]
        hsz, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        _need(len(b) >= hsz, "literals header past the block")
        h = int.from_bytes(b[:hsz], "little")
        regen, csize = (h >> 4) & ((1 << bits) - 1), (h >> (4 + bits)) & ((1 << bits) - 1)
        c[f"lit/{name}/sf{sf}"] += 1
        size = hsz + csize
        if kind == 2:
            _need(len(b) > hsz, "no Huffman tree header")
            hb = b[hsz]
            tree = 1 + (hb if hb < 128 else (hb - 127 + 1) // 2)
            c["hufhdr/fse" if hb < 128 else "hufhdr/direct"] += 1
            _need(tree + (6 if sf else 0) < csize, "Huffman tree description does not fit its section")
    _need(regen <= BLOCK_MAX, "literals larger than a block")
    _need(size <= len(b), "literals section past the block")
    if regen == 0:
        c["lit/regen=0"] += 1
    return size, regen


def _sequences(c, b: bytes, reserved_ok=False):
    """the sequences section (the rest of a block): its count; the tables and the bitstream are not decoded"""
    _need(len(b) >= 1, "no sequences section")
    b0 = b[0]
    if b0 == 0:
        _need(len(b) == 1, "bytes after an empty sequences section")
        c["nseq/0"] += 1
        return 0
    if b0 < 128:
        nseq, p = b0, 1
    elif b0 < 255:
        _need(len(b) >= 2, "sequence count past the block")
        nseq, p = ((b0 - 128) << 8) + b[1], 2
    else:
        _need(len(b) >= 3, "sequence count past the block")
        nseq, p = b[1] + (b[2] << 8) + 0x7F00, 3
    c["nseq/1-127" if p == 1 else "nseq/128-32511" if p == 2 else "nseq/long"] += 1
    _need(len(b) > p, "no table-mode byte")
    m = b[p]
    _need(reserved_ok or not m & 3, "reserved table-mode bits")
    rle = 0
    for name, shift in (("LL", 6), ("OF", 4), ("ML", 2)):
        mode = (m >> shift) & 3
        c[f"{name}/{MODES[mode]}"] += 1
        rle += mode == 1
    _need(len(b) >= p + 1 + rle + 1, "no room for the RLE symbols and the bitstream")
    _need(b[-1] != 0, "the bitstream's last byte has no end mark")
    return nseq


def walk(frame: bytes, reserved_ok=False):
    """(Counter of classes, [(regen_size, nseq) per compressed block], content size or None); reserved_ok: the two
    reserved bits of a table-mode byte may be set (zstd 1.5.2 does not look at them)"""
    frame = bytes(frame)
    c = Counter()
    p, fcs, checksum = frame_header(frame)
    blocks, nblocks, total = [], 0, 0
    while True:
        _need(p + 3 <= len(frame), "block header past the end")
        bh = int.from_bytes(frame[p:p + 3], "little")
        p += 3
        last, btype, bsz = bh & 1, (bh >> 1) & 3, bh >> 3
        nblocks += 1
        _need(btype != 3, "reserved block type")
        _need(bsz <= BLOCK_MAX, "block larger than 128 KiB")
        if btype == 0:
            c["block/raw"] += 1
            total += bsz
            p += bsz
        elif btype == 1:
            c["block/rle"] += 1
            total += bsz
            p += 1
        else:
            c["block/cmp"] += 1
            _need(p + bsz <= len(frame), "compressed block past the end")
            body = frame[p:p + bsz]
            lsz, regen = _literals(c, body)
            nseq = _sequences(c, body[lsz:], reserved_ok)
            blocks.append((regen, nseq))
            p += bsz
        _need(p <= len(frame), "block past the end")
        if last:
            break
    c["blocks/1" if nblocks == 1 else "blocks/2+"] += 1
    p += 4 if checksum else 0
    _need(p == len(frame), f"the walk ends at byte {p} of {len(frame)}")
    if not blocks and fcs is not None:
        _need(total == fcs, "raw and RLE blocks do not add up to the content size")
    return c, blocks, fcs


def census(frame: bytes) -> Counter:
    return walk(frame)[0]


def frames_of(packed, csizes, n: int, chunk: int):
    """(frame bytes, chunk bytes) for every chunk of an lzbench-packed stream that is a frame: a chunk whose
    packed size equals its own size is stored raw and is no frame"""
    packed = bytes(memoryview(packed))
    pos = 0
    for i, s in enumerate(csizes):
        s = int(s)
        part = min(chunk, n - i * chunk)
        if s != part:
            yield packed[pos:pos + s], part
        pos += s
    assert pos == len(packed)


def census_packed(packed, csizes, n: int, chunk: int):
    """(Counter, [(content size, [(regen, nseq), ...]) per frame]) over a packed stream; every frame's content
    size must be its chunk's"""
    c, per = Counter(), []
    for f, part in frames_of(packed, csizes, n, chunk):
        cc, blocks, fcs = walk(f)
        _need(fcs == part, f"content size {fcs} of a {part}-byte chunk")
        c.update(cc)
        per.append((part, blocks))
    return c, per


def long_match_frames(per):
    """frames (of census_packed's list) of one block and one sequence whose match is 65539 bytes or longer: the
    match-length code 52 with all 16 extra bits in use (ML_base[52] = 65539)"""
    return [(n, b) for n, b in per if len(b) == 1 and b[0][1] == 1 and n - b[0][0] >= 65539]


def long_literal_frames(per):
    """frames of one block, one sequence and 65536 literals or more.  The literals are split between the
    sequence's literal length and the block's tail; for the sequence to carry LL code 35 (LL_base[35] = 65536)
    the caller's input must put them all before the match."""
    return [(n, b) for n, b in per if len(b) == 1 and b[0][1] == 1 and b[0][0] >= 65536]
