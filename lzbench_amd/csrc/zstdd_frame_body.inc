// lzbench_amd/csrc/zstdd_frame_body.inc -- body of the one-wave-per-frame zstd decoders (lzh_zstd_decompress_kernel,
// decode_hip.hip; lzh_zstd_decompress_ragged_sel_kernel, zstd_ragged_split_hip.hip) after the frame lookup.  The
// including kernel has: L (its LDS), lane, chunk, out + ooff (the frame's output address), part (its size), packed,
// packed_readable, offsets, csizes, status, stats.
// Textual, not a function: see zstdd_hdr_body.inc.
    const uint64_t ioff = offsets[chunk];
    const int cs = (int)csizes[chunk];
    // (+16: whole-dword reads of the frame's last bytes; bytes past the frame are never used)
    const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, (uint64_t)cs + 16) : 0;
    Bytes rin, rout;
    rin.init(packed + ioff, readable);
    rout.init(out + ooff, (uint64_t)part);
    int r;
    if (cs == part) {                                  // stored raw by the chunk loop (lzbench.cpp:284-288)
        copy_raw(rin, rout, part, lane);
        r = part;
    } else {
        zstdd::ZSink O{(LDSA uint8_t*)L.win, rout, 0, 0};
        for (int i = lane; i < 36 + 53; i += LZH_WAVE) L.base[i] = i < 36 ? zstdd::kLLBase[i] : zstdd::kMLBase[i - 36];
        wave_lds_fence();
        Bytes lout;
        lout.init(out + ooff, (uint64_t)part + 3);
        r = zstdd::decode_frame(rin, lout, cs, O, L, part, lane, stats);
        if (r > 0) O.flush(r, lane);
    }
    if (lane == 0) status[chunk] = r;
