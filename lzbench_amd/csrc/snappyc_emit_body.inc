// lzbench_amd/csrc/snappyc_emit_body.inc -- body of sne::emit_chunk (snappyc_hip.hip) and sne::emit_ragged
// (ragged_hip.hip) after the chunk lookup.  The including function has: kMulti, lane, wave, W, chunk (its index),
// in + off (its address), in_readable - off (bytes that may be read from there), n (its size), rings, ibufs, fsz
// (LDS), recs, rec_stride, rec_hdr, stage, stride, csizes, frags.  Textual, not a function: see
// snappyc_parse_body.inc.
    LDSA uint8_t* ring = rings + wave * kRingB;
    LDSA uint32_t* ibuf = ibufs + wave * kSpanDw;
    Bytes in_b;
    in_b.init(in + off, min<uint64_t>(in_readable - off, (uint64_t)n + 64));
    const rsrc_t rr = make_rsrc(recs + chunk * rec_stride, (uint32_t)rec_stride);
    const uint32_t* hdr = rec_hdr + chunk * frags;
    const int nf = (int)((n + 65535u) >> 16);
    const rsrc_t so = make_rsrc(stage + chunk * stride, (uint32_t)stride);
    int nb = 1;                                    // varint32 uncompressed length (snappy.cc:1047-1050)
    for (uint32_t v = n; v >= 128; v >>= 7) nb++;
    if constexpr (!kMulti) {   // one fragment (chunks of at most 64 KiB)
        OutR<false> R{ring, so, 0};
        if (lane < nb) R.put(lane, ((n >> (7 * lane)) & 0x7fu) | (lane + 1 < nb ? 0x80u : 0u));
        const int e = emit_records(R, in_b, rr, 0, (int)uni(hdr[0]), 0, nb, ibuf, lane);
        R.flush(e, true, lane);
        if (lane == 0) csizes[chunk] = (uint32_t)e;
    } else {
    // sizes of all fragments but the last (the last one's end is the chunk's compressed size)
    for (int f = wave; f < nf - 1; f += W) {
        const int r0 = f * kFragRecs, r1 = (int)uni(hdr[f]);
        const int bytes = frag_bytes(rr, r0, r1, f << 16, lane);
        if (lane == 0) fsz[f] = (uint32_t)bytes;
    }
    if (kMulti) __syncthreads();
    // the varint goes through fragment 0's ring (an empty chunk: a store of its own)
    const uint32_t vb = ((n >> (7 * lane)) & 0x7fu) | (lane + 1 < nb ? 0x80u : 0u);
    if (nf == 0 && wave == 0) {
        if (lane < nb) st_u8(so, lane, vb);
        if (lane == 0) csizes[chunk] = (uint32_t)nb;
    }
    int base = nb;
    for (int f = 0; f < nf; f++) {
        if ((f % W) == wave) {
            const int r0 = f * kFragRecs, r1 = (int)uni(hdr[f]);
            OutR<kMulti> R{ring, so, f == 0 ? 0 : base};
            if (f == 0 && lane < nb) R.put(lane, vb);
            const int e = emit_records(R, in_b, rr, r0, r1, f << 16, base, ibuf, lane);
            R.flush(e, true, lane);
            if (f == nf - 1 && lane == 0) csizes[chunk] = (uint32_t)e;
        }
        if (f < nf - 1) base += (int)uni(((volatile LDSA uint32_t*)fsz)[f]);
    }
    }
