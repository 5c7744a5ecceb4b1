"""tests/lz_census.py -- which constructs of the LZ4 block format and of the snappy format a stream uses.  Pure
Python, no GPU; the counterpart of tests/zstd_census.py.

lz4(stream, cap, prefix=0) and snappy(stream, cap) walk one stream token by token with the acceptance rules of the
reference decoders (LZ4_decompress_safe, snappy::RawUncompress) and return a Counter of the classes below;
anything those decoders reject raises CensusError.  Both also return the decoded size.  No bytes are decoded, and a
class is a property of the stream (and of the capacity it is decoded with) alone: nothing here models how a decoder
kernel groups tokens.

KW is a decoder kernel's output window, 4096, 8192 or 16384 bytes; EDGES(KW) are the offsets where a source is
the last one inside a window or the first one outside it.

  both codecs (C = lz4 or snappy)
    C/off/KW-129@KW, C/off/KW-128@KW, C/off/KW-127@KW, C/off/KW@KW, C/off/KW+1@KW   a match at that offset
    C/off/thr@KW                a match at an offset of KW-127 .. KW-1: whether its source is still in the window
                                depends on where the byte falls in a 128-byte pass of the group emitter
    C/match-after-bulk-lit      a match at offset 1..63 right after more than 512 literal bytes
    C/short-of-cap              the stream decodes to fewer bytes than the capacity
  LZ4
    lz4/run3x21                 21 or more consecutive 3-byte sequences (no literals, match length 4..18)
    lz4/match>window@KW         a match longer than KW at one of EDGES(KW) or in the thr band
    lz4/overlap>window@KW       a match at an offset under 64 (a period shorter than a wave) that is not a power of
                                two, long enough to come round the window onto its own source (KW - offset bytes)
    lz4/ll-run255, lz4/ml-run255  a literal / match length with a length byte of 255
    lz4/prefix-overlap          (linked blocks) a match that starts in the prefix and runs into the block
    lz4/limit/cap-12, /cs-8, /cap-5, /cs-15, /cs-4   a sequence exactly on that end-of-block limit
    lz4/off=pos                 a match whose source is the first byte there is
    lz4/off=0                   offset 0, which LZ4_decompress_safe accepts (counted, used by no case)
  snappy
    snappy/copy1, /copy2, /copy4, snappy/lit/len0 .. /len4   the tag kinds and literal length forms
    snappy/copy2/short          a COPY_2 that a COPY_1 could hold, or of fewer than 4 bytes
    snappy/copy/len1            a copy of one byte
    snappy/lit/noncanonical     a literal with more length bytes than its length needs
    snappy/lit/consecutive      a literal tag right after a literal tag, inside a 64 KiB fragment (an encoder that
                                works a fragment at a time ends one and starts the next with a literal)
    snappy/run2x32              32 or more consecutive two-byte tags (1-byte literals, COPY_1s)
    snappy/off>65535            a COPY_4 offset no COPY_2 holds
    snappy/copy/cross-fragment  a copy whose source starts before the 64 KiB fragment its first byte is in
    snappy/tag-at-fragment      a tag that starts at a positive multiple of 64 KiB of output
    snappy/off=pos              a copy whose source is the first byte there is"""
from collections import Counter

WINDOWS = (4096, 8192, 16384)
FRAGMENT = 65536


class CensusError(ValueError):
    pass


def _need(cond, what):
    if not cond:
        raise CensusError(what)


def EDGES(kw):
    return (kw - 129, kw - 128, kw - 127, kw, kw + 1)


EDGE_NAMES = ("KW-129", "KW-128", "KW-127", "KW", "KW+1")
ALL_EDGE_OFFSETS = sorted({o for kw in WINDOWS for o in EDGES(kw)})


def off_classes(codec, off):
    out = []
    for kw in WINDOWS:
        for name, o in zip(EDGE_NAMES, EDGES(kw)):
            if off == o:
                out.append(f"{codec}/off/{name}@{kw}")
        if kw - 127 <= off <= kw - 1:
            out.append(f"{codec}/off/thr@{kw}")
    return out


LZ4_CLASSES = ([c for kw in WINDOWS for o in EDGES(kw) for c in off_classes("lz4", o) if "thr" not in c]
               + [f"lz4/off/thr@{kw}" for kw in WINDOWS] + [f"lz4/match>window@{kw}" for kw in WINDOWS]
               + [f"lz4/overlap>window@{kw}" for kw in WINDOWS]
               + ["lz4/run3x21", "lz4/ll-run255", "lz4/ml-run255", "lz4/match-after-bulk-lit", "lz4/short-of-cap",
                  "lz4/prefix-overlap", "lz4/limit/cap-12", "lz4/limit/cs-8", "lz4/limit/cap-5", "lz4/limit/cs-15",
                  "lz4/limit/cs-4", "lz4/off=pos"])
SNAPPY_CLASSES = ([c for kw in WINDOWS for o in EDGES(kw) for c in off_classes("snappy", o) if "thr" not in c]
                  + [f"snappy/off/thr@{kw}" for kw in WINDOWS]
                  + ["snappy/copy1", "snappy/copy2", "snappy/copy4"] + [f"snappy/lit/len{i}" for i in range(5)]
                  + ["snappy/copy2/short", "snappy/copy/len1", "snappy/lit/noncanonical", "snappy/lit/consecutive",
                     "snappy/run2x32", "snappy/off>65535", "snappy/copy/cross-fragment", "snappy/tag-at-fragment",
                     "snappy/match-after-bulk-lit", "snappy/short-of-cap", "snappy/off=pos"])


def lz4(stream: bytes, cap: int, prefix: int = 0):
    """(Counter, decoded size) of an LZ4 block decoded with capacity cap after `prefix` bytes of earlier output
    (LZ4_decompress_safe, lz4.c:1929-2151; with a prefix, LZ4_decompress_safe_usingDict)"""
    c = Counter()
    cs = len(stream)
    if cap == 0:
        _need(cs == 1 and stream[0] == 0, "lz4: an empty block is one zero token")
        return c, 0
    _need(cs > 0, "lz4: empty stream")
    ip = op = run3 = 0
    while True:
        _need(ip < cs, "lz4: token past the end")
        tok_at = ip
        tok = stream[ip]
        ip += 1
        lit = tok >> 4
        if lit == 15:
            _need(ip < cs - 15, "lz4: literal length bytes past cs - 15")
            if ip == cs - 16:
                c["lz4/limit/cs-15"] += 1
            while True:
                s = stream[ip]
                ip += 1
                lit += s
                if s == 255:
                    c["lz4/ll-run255"] += 1
                if ip >= cs - 15 or s != 255:   # (the reference stops there without an error, lz4.c:1967-1970)
                    break
        if op + lit > cap - 12 or ip + lit > cs - 8:
            _need(ip + lit == cs and op + lit <= cap, "lz4: a last sequence that does not end the block")
            op += lit
            break
        if op + lit == cap - 12:
            c["lz4/limit/cap-12"] += 1
        if ip + lit == cs - 8:
            c["lz4/limit/cs-8"] += 1
        ip += lit
        op += lit
        off = stream[ip] | stream[ip + 1] << 8
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                s = stream[ip]
                ip += 1
                ml += s
                _need(ip < cs - 4, "lz4: match length bytes past cs - 4")
                if s == 255:
                    c["lz4/ml-run255"] += 1
                if s != 255:
                    if ip == cs - 5:
                        c["lz4/limit/cs-4"] += 1
                    break
        ml += 4
        _need(off <= op + prefix, "lz4: offset before the first byte")
        _need(op + ml <= cap - 5, "lz4: match past cap - 5")
        if op + ml == cap - 5:
            c["lz4/limit/cap-5"] += 1
        if off == 0:   # (accepted by the reference: the match reads the destination as it was)
            c["lz4/off=0"] += 1
        c.update(off_classes("lz4", off))
        for kw in WINDOWS:
            if ml > kw and kw - 129 <= off <= kw + 1:
                c[f"lz4/match>window@{kw}"] += 1
            if 0 < off < 64 and off & (off - 1) and ml > kw - off:
                c[f"lz4/overlap>window@{kw}"] += 1
        if off == op + prefix:
            c["lz4/off=pos"] += 1
        if off > op and off < op + ml:
            c["lz4/prefix-overlap"] += 1
        if lit > 512 and off <= 63:
            c["lz4/match-after-bulk-lit"] += 1
        run3 = run3 + 1 if ip - tok_at == 3 else 0
        if run3 == 21:
            c["lz4/run3x21"] += 1
        op += ml
    if op < cap:
        c["lz4/short-of-cap"] += 1
    return c, op


def snappy(stream: bytes, cap: int):
    """(Counter, decoded size) of a snappy stream decoded into cap bytes (snappy.cc:848-1036, :1319-1407)"""
    c = Counter()
    cs = len(stream)
    ip = ulen = shift = 0
    while True:
        _need(ip < cs and shift < 32, "snappy: varint")
        b = stream[ip]
        ip += 1
        _need(not (shift == 28 and (b & 0x7f) > 15), "snappy: varint above 32 bits")
        ulen |= (b & 0x7f) << shift
        shift += 7
        if b < 128:
            break
    _need(ulen <= cap, "snappy: length above the capacity")
    op = run2 = 0
    prev_lit = False
    while ip < cs:
        t = stream[ip]
        at = ip
        ip += 1
        kind = t & 3
        if kind == 0:
            ln = (t >> 2) + 1
            nb = 0
            if ln > 60:
                nb = ln - 60
                _need(ip + nb <= cs, "snappy: literal length bytes past the end")
                ln = int.from_bytes(stream[ip:ip + nb], "little") + 1
                ip += nb
            _need(ip + ln <= cs and op + ln <= ulen, "snappy: literal past the end")
            c[f"snappy/lit/len{nb}"] += 1
            need = 0 if ln <= 60 else (ln - 1).bit_length() + 7 >> 3
            if nb > need:
                c["snappy/lit/noncanonical"] += 1
            if op and op % FRAGMENT == 0:
                c["snappy/tag-at-fragment"] += 1
            elif prev_lit:
                c["snappy/lit/consecutive"] += 1
            prev_lit = True
            bulk = ln > 512
            ip += ln
            op += ln
        else:
            extra = (0, 1, 2, 4)[kind]
            _need(ip + extra <= cs, "snappy: copy tag past the end")
            if kind == 1:
                ln = ((t >> 2) & 7) + 4
                off = (t >> 5) << 8 | stream[ip]
            else:
                ln = (t >> 2) + 1
                off = int.from_bytes(stream[ip:ip + extra], "little")
            ip += extra
            _need(0 < off <= op and op + ln <= ulen, "snappy: copy out of range")
            c[f"snappy/copy{extra}"] += 1
            if kind == 2 and (ln < 4 or (off < 2048 and ln <= 11)):
                c["snappy/copy2/short"] += 1
            if ln == 1:
                c["snappy/copy/len1"] += 1
            if off > 65535:
                c["snappy/off>65535"] += 1
            if op - off < op // FRAGMENT * FRAGMENT:
                c["snappy/copy/cross-fragment"] += 1
            if op % FRAGMENT == 0:
                c["snappy/tag-at-fragment"] += 1
            if off == op:
                c["snappy/off=pos"] += 1
            if prev_lit and bulk and off <= 63:
                c["snappy/match-after-bulk-lit"] += 1
            c.update(off_classes("snappy", off))
            prev_lit = False
            op += ln
        run2 = run2 + 1 if ip - at == 2 else 0
        if run2 == 32:
            c["snappy/run2x32"] += 1
    _need(op == ulen, "snappy: the tags do not produce the announced length")
    if op < cap:
        c["snappy/short-of-cap"] += 1
    return c, op


def census(codec, stream, cap, prefix=0):
    return lz4(stream, cap, prefix)[0] if codec == "lz4" else snappy(stream, cap)[0]
