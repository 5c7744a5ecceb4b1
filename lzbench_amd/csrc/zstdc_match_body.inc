// lzbench_amd/csrc/zstdc_match_body.inc -- body of the zstd match kernels (lzh_zstd_match_kernel, zstdc_hip.hip;
// lzh_zstd_match_ragged_kernel, zstd_ragged_hip.hip) after the frame lookup.  The including kernel has: zlds (the
// dynamic LDS), lane, f (the frame's index: its scratch area), in + ioff (the frame's address), in_readable - ioff
// (bytes that may be read from there), nf (its size), chunk_size (the largest frame of the launch: it selects the
// table kind with lds_arg), level, k (the block), scratch, fstride, seq_off, lit_off, tab_off, lds_arg.
// Textual, not a function: the uniform kernel's code must stay bit-identical (profiles are keyed to kernel code
// hashes).
    const ZParams P = params_for(level, nf);
    if (!P.ok) return;
    const uint64_t nblocks = nf ? (nf + P.bsize - 1) / P.bsize : 1;
    if ((uint64_t)k >= nblocks) return;
    uint8_t* fs = scratch + f * fstride;
    rsrc_t hdr = make_rsrc(fs, 64);
    const int bs = k * (int)P.bsize;
    const int be = (int)min<uint64_t>(nf, (uint64_t)bs + P.bsize);
    if (be - bs < 7) {                                   // ZSTD_buildSeqStore: too small, stored raw
        if (lane == 0) { st_b32(hdr, 32, 1u); st_b32(hdr, 0, 0u); st_b32(hdr, 4, 0u); }
        return;
    }
    Bytes in_b;
    in_b.init(in + ioff, min<uint64_t>(in_readable - ioff, nf + 16));
    SeqOut O;
    O.seq = make_rsrc(fs + seq_off, (uint32_t)(lit_off - seq_off));
    O.lits.init(fs + lit_off, P.bsize + 64);
    O.ns = 0;
    O.nl = 0;
    uint32_t rep[2] = {1u, 4u};                          // repStartValue
    if (k > 0) { rep[0] = uni(ld_b32(hdr, 16)); rep[1] = uni(ld_b32(hdr, 20)); }
    const uint32_t tbytes = 4u << P.hlog;
    const uint32_t nent = 1u << P.hlog;
    const uint32_t lds_table_bytes = lds_arg;          // the table's bytes in dynamic LDS (0: global)
    const uint32_t bmb = max(nent / 8u, 4u);            // LdsTab17 bitmap bytes
    if (chunk_size <= 131072u && nblocks == 1 && 2u * nent + bmb <= lds_table_bytes) {
        // (single-block frames: the table starts empty and is not saved)
        LdsTab17 T{(LDSA uint16_t*)zlds, (LDSA uint32_t*)((LDSA uint8_t*)zlds + 2 * nent)};
        for (uint32_t i = lane; i < (2u * nent + bmb) / 4u; i += 64) ((volatile LDSA uint32_t*)zlds)[i] = 0u;
        T.fence();
        if (P.mls == 6) fast_block<6>(T, in_b, P, bs, be, rep, O, lane);   // (hash fixed at compile time)
        else if (P.mls == 5) fast_block<5>(T, in_b, P, bs, be, rep, O, lane);
        else fast_block(T, in_b, P, bs, be, rep, O, lane);
    } else if (chunk_size < (16u << 20) && 3u * nent <= lds_table_bytes) {
        LdsTab24 T{(LDSA uint16_t*)zlds, (LDSA uint8_t*)zlds + 2 * nent};
        rsrc_t save = make_rsrc(fs + tab_off, tbytes);
        for (uint32_t i = lane; i < nent; i += 64) T.put(i, k == 0 ? 0u : ld_b32(save, (int)(i * 4)));
        T.fence();
        fast_block(T, in_b, P, bs, be, rep, O, lane);
        if ((uint64_t)k + 1 < nblocks)
            for (uint32_t i = lane; i < nent; i += 64) st_b32(save, (int)(i * 4), T.get(i));
    } else if (tbytes <= lds_table_bytes) {
        LdsTab T{(LDSA uint32_t*)zlds};
        rsrc_t save = make_rsrc(fs + tab_off, tbytes);
        for (uint32_t i = lane; i < tbytes / 4; i += 64) T.put(i, k == 0 ? 0u : ld_b32(save, (int)(i * 4)));
        T.fence();
        fast_block(T, in_b, P, bs, be, rep, O, lane);
        if ((uint64_t)k + 1 < nblocks)
            for (uint32_t i = lane; i < tbytes / 4; i += 64) st_b32(save, (int)(i * 4), T.get(i));
    } else {
        GlbTab T{make_rsrc(fs + tab_off, tbytes)};
        if (k == 0) {
            for (uint32_t i = lane; i < tbytes / 4; i += 64) T.put(i, 0u);
            T.fence();
        }
        fast_block(T, in_b, P, bs, be, rep, O, lane);
    }
    if (lane == 0) {
        st_b32(hdr, 0, (uint32_t)O.ns);
        st_b32(hdr, 4, (uint32_t)O.nl);
        st_b32(hdr, 8, rep[0]);
        st_b32(hdr, 12, rep[1]);
        st_b32(hdr, 32, 0u);
    }
