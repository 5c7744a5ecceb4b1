// lzbench_amd/csrc/zstdc_dfast_match_body.inc -- body of the zstd level-3 match kernels (lzh_zstd_dfast_match_kernel,
// zstdc_dfast_hip.hip; lzh_zstd_dfast_match_ragged_kernel and lzh_zstd_dfast_match_compact_kernel,
// zstd_dfast_ragged_hip.hip) after the frame lookup.  The including kernel has: lane, f (the frame's index: its
// scratch area), in + ioff (the frame's address), in_readable - ioff (bytes that may be read from there), nf (its
// size), level, k (the block), scratch, fstride, seq_off, lit_off, tab_off (the long table; the short one follows it).
// The frame's parameters, its two tables' sizes included, come from nf alone.
// Textual, not a function: the uniform kernel's code must stay bit-identical (profiles are keyed to kernel code
// hashes).
    const zdf::DParams P = zdf::params_for(level, nf);
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
    const uint32_t lbytes = 4u << P.hlog, sbytes = 4u << P.clog;
    zdf::WaveEnv E{in_b, GlbTab{make_rsrc(fs + tab_off, lbytes)}, GlbTab{make_rsrc(fs + tab_off + lbytes, sbytes)}, O, lane};
    if (k == 0) {                                        // both tables start empty per frame
        rsrc_t both = make_rsrc(fs + tab_off, lbytes + sbytes);
        for (uint32_t i = lane; i < (lbytes + sbytes) / 4; i += 64) st_b32(both, (int)(i * 4), 0u);
        E.fence();
    }
    const int anchor = zdf::dfast_block(E, P, bs, be, rep);
    copy_span(in_b, anchor, O.lits, O.nl, be - anchor, lane, LZH_WAVE);   // last literals
    O.nl += be - anchor;
    if (lane == 0) {
        st_b32(hdr, 0, (uint32_t)O.ns);
        st_b32(hdr, 4, (uint32_t)O.nl);
        st_b32(hdr, 8, rep[0]);
        st_b32(hdr, 12, rep[1]);
        st_b32(hdr, 32, 0u);
    }
