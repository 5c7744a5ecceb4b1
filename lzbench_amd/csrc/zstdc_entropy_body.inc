// lzbench_amd/csrc/zstdc_entropy_body.inc -- body of the zstd entropy kernels (lzh_zstd_entropy_kernel,
// zstdc_hip.hip; lzh_zstd_entropy_ragged_kernel, zstd_ragged_hip.hip) after the frame lookup.  The including kernel
// has: L (its ze::Lds), lane, f (the frame's index: its scratch area, staging slot and csizes entry), in + ioff (the
// frame's address), in_readable - ioff (bytes that may be read from there), nf (its size), level, k (the block),
// scratch, fstride, seq_off, lit_off, att_off, tmp_off, stage, stride, csizes.
// Textual, not a function: the uniform kernel's code must stay bit-identical (profiles are keyed to kernel code
// hashes).
    const ZParams P = params_for(level, nf);
    if (!P.ok) return;
    const uint64_t nblocks = nf ? (nf + P.bsize - 1) / P.bsize : 1;
    if ((uint64_t)k >= nblocks) return;
    uint8_t* fs = scratch + f * fstride;
    rsrc_t hdr = make_rsrc(fs, 1024);
    Bytes out;
    out.init(stage + f * stride, stride);
    int out_off;
    if (k == 0) {
        // ZSTD_writeFrameHeader (zstd_compress.c:4012-4058): single segment, content size, no checksum
        const uint64_t wsize = 1ull << P.wlog;
        const int single = wsize >= nf;
        const int fcs = (nf >= 256) + (nf >= 65536 + 256) + (nf >= 0xFFFFFFFFull);
        int o = 0;
        if (lane == 0) {
            out.st8(0, 0x28); out.st8(1, 0xB5); out.st8(2, 0x2F); out.st8(3, 0xFD);
            out.st8(4, (uint32_t)((single << 5) + (fcs << 6)));
        }
        o = 5;
        if (!single) { if (lane == 0) out.st8(o, (P.wlog - 10) << 3); o++; }
        if (lane == 0) {
            if (fcs == 0) { if (single) out.st8(o, (uint32_t)nf & 0xff); }
            else if (fcs == 1) { const uint32_t v = (uint32_t)(nf - 256); out.st8(o, v & 0xff); out.st8(o + 1, v >> 8); }
            else if (fcs == 2) { for (int i = 0; i < 4; i++) out.st8(o + i, (uint32_t)(nf >> (8 * i)) & 0xff); }
            else { for (int i = 0; i < 8; i++) out.st8(o + i, (uint32_t)(nf >> (8 * i)) & 0xff); }
        }
        o += fcs == 0 ? (single ? 1 : 0) : (fcs == 1 ? 2 : (fcs == 2 ? 4 : 8));
        out_off = o;
        if (lane == 0) { st_b32(hdr, 16, 1u); st_b32(hdr, 20, 4u); st_b32(hdr, 24, 0u); }
    } else {
        out_off = (int)uni(ld_b32(hdr, 28));
    }
    if (nf == 0) {                                        // ZSTD_writeEpilogue: empty last raw block
        if (lane == 0) { out.st8(out_off, 1); out.st8(out_off + 1, 0); out.st8(out_off + 2, 0); csizes[f] = (uint32_t)out_off + 3; }
        return;
    }
    const int bs = k * (int)P.bsize;
    const int be = (int)min<uint64_t>(nf, (uint64_t)bs + P.bsize);
    const int len = be - bs;
    const int last = (uint64_t)be == nf;
    Bytes in_b;
    in_b.init(in + ioff, min<uint64_t>(in_readable - ioff, nf + 16));
    const int skip = len < 7 || uni(ld_b32(hdr, 32)) != 0u;
    int csize = 0, newTable = 0;
    Bytes att;
    att.init(fs + att_off, tmp_off - att_off);
    if (!skip) {
        const int ns = (int)uni(ld_b32(hdr, 0)), nl = (int)uni(ld_b32(hdr, 4));
        const int prevRepeat = (int)uni(ld_b32(hdr, 24));
        if (prevRepeat) {
            rsrc_t ht = make_rsrc(fs + zc::kHufOff, 768);
            for (int s = lane; s < 256; s += 64) {
                L.pnb[s] = (uint8_t)ld_u8(ht, s);
                L.pval[s] = (uint16_t)(ld_u8(ht, 256 + 2 * s) | (ld_u8(ht, 257 + 2 * s) << 8));
            }
            wave_lds_fence();
        }
        Bytes lits, tmp;
        lits.init(fs + lit_off, P.bsize + 64);
        tmp.init(fs + tmp_off, P.bsize + 256);
        int o = ze::compress_literals(L, att, tmp, lits, nl, ns, P, prevRepeat, newTable, lane);
        if (lane == 0) {
            if (ns < 128) att.st8(o, (uint32_t)ns);
            else if (ns < 0x7F00) { att.st8(o, (uint32_t)((ns >> 8) + 0x80)); att.st8(o + 1, (uint32_t)ns & 0xff); }
            else { att.st8(o, 0xFF); att.st8(o + 1, (uint32_t)(ns - 0x7F00) & 0xff); att.st8(o + 2, (uint32_t)(ns - 0x7F00) >> 8); }
        }
        o += ns < 128 ? 1 : (ns < 0x7F00 ? 2 : 3);
        if (ns) {
            const int sz = ze::encode_sequences(L, att, tmp, o, make_rsrc(fs + seq_off, (uint32_t)(lit_off - seq_off)), ns, lane);
            csize = sz ? o + sz : 0;
        } else {
            csize = o;
        }
        if (csize && csize >= len - ((len >> 6) + 2)) csize = 0;   // ZSTD_minGain
    }
    if (len >= 7 && k > 0 && csize < 25) {                          // RLE block (not for the first block)
        const uint32_t b0 = in_b.b(bs);
        bool diff = false;
        for (int i = lane; i < len; i += 64) diff |= in_b.b(bs + i) != b0;
        if (!ballot(diff)) csize = 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int bsz;
    if (csize == 0) {
        if (lane == 0) { const uint32_t h = (uint32_t)last + ((uint32_t)len << 3); out.st8(out_off, h & 0xff); out.st8(out_off + 1, (h >> 8) & 0xff); out.st8(out_off + 2, h >> 16); }
        copy_span(in_b, bs, out, out_off + 3, len, lane, 64);
        bsz = 3 + len;
    } else if (csize == 1) {
        if (lane == 0) {
            const uint32_t h = (uint32_t)last + (1u << 1) + ((uint32_t)len << 3);
            out.st8(out_off, h & 0xff); out.st8(out_off + 1, (h >> 8) & 0xff); out.st8(out_off + 2, h >> 16);
            out.st8(out_off + 3, in_b.b(bs));
        }
        bsz = 4;
    } else {
        if (lane == 0) { const uint32_t h = (uint32_t)last + (2u << 1) + ((uint32_t)csize << 3); out.st8(out_off, h & 0xff); out.st8(out_off + 1, (h >> 8) & 0xff); out.st8(out_off + 2, h >> 16); }
        copy_span(att, 0, out, out_off + 3, csize, lane, 64);
        bsz = 3 + csize;
        // confirm repcodes and the Huffman table (ZSTD_blockState_confirmRepcodesAndEntropyTables)
        if (lane == 0) { st_b32(hdr, 16, ld_b32(hdr, 8)); st_b32(hdr, 20, ld_b32(hdr, 12)); }
        if (newTable) {
            rsrc_t ht = make_rsrc(fs + zc::kHufOff, 768);
            for (int s = lane; s < 256; s += 64) {
                st_u8(ht, s, L.nb[s]);
                st_u8(ht, 256 + 2 * s, L.val[s] & 0xff);
                st_u8(ht, 257 + 2 * s, L.val[s] >> 8);
            }
            if (lane == 0) st_b32(hdr, 24, 1u);
        }
    }
    out_off += bsz;
    if (lane == 0) {
        st_b32(hdr, 28, (uint32_t)out_off);
        if (last) csizes[f] = (uint32_t)out_off;
    }
