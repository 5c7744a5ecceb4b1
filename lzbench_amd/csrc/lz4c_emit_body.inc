// lzbench_amd/csrc/lz4c_emit_body.inc -- body of the LZ4 emit kernels (lzh_lz4_emit_kernel, lz4c_hip.hip;
// lzh_lz4_emit_ragged_kernel, ragged_hip.hip) after the chunk lookup.  The including kernel has: lane, chunk (its
// index), n (its size), in_b (its bytes), ring and ibuf (LDS), recs, rec_stride, rec_hdr, stage, stride, csizes.
// Textual, not a function: see lz4c_parse_body.inc.
    const rsrc_t rr = make_rsrc(recs + chunk * rec_stride, (uint32_t)rec_stride);
    const int nrec = (int)uni(rec_hdr[2 * chunk]);
    lz4e::OutR R{(LDSA uint8_t*)ring, make_rsrc(stage + chunk * stride, (uint32_t)stride), 0};
    // Software pipeline over groups of 64 records: while group g is laid out, the loads of group g+1
    // (its input span and catch-up words) and the records of group g+2 are in flight, so a group's one
    // memory wait comes a whole group after its loads were issued.
    int op = 0, ia_end = 0;
    lz4e::Grp GA, GB;                           // headers of groups g and g+1 (alternating roles)
    uint32_t sp[lz4e::kSpanW], cw[4];           // group g's span and catch-up dwords (in flight)
    // records of group g+1 (in flight), per lane; past nrec the offsets are out of range (0)
    uint32_t nw0 = ld_b32(rr, 8 * (64 + lane)), nw1 = ld_b32(rr, 8 * (64 + lane) + 4);
    {
        const uint32_t w0 = ld_b32(rr, 8 * lane), w1 = ld_b32(rr, 8 * lane + 4);
        GA.head(w0, w1, 0, 0, nrec, in_b, lane);
        GA.issue(in_b, lane, cw, sp);
    }
    auto step = [&](lz4e::Grp& G, lz4e::Grp& Gn, int g) {
        // group g's input span into LDS (literal bytes are read from it), its catch-up words
        if (G.span) {
#pragma unroll
            for (int k = 0; k < lz4e::kSpanW; k++)
                if (64 * k < G.nd && lane + 64 * k < G.nd) ibuf[lane + 64 * k] = sp[k];
            wave_lds_fence();
        }
        const uint32_t xp = lz4e::Grp::before(cw[0], cw[1], G.Pm, in_b.sh);
        const uint32_t xm = lz4e::Grp::before(cw[2], cw[3], G.Pm - G.o, in_b.sh);
        // group g+1: header from its records; its loads and the records of group g+2 go out now
        {
            const uint32_t w0 = nw0, w1 = nw1;
            nw0 = ld_b32(rr, 8 * (g + 128 + lane));
            nw1 = ld_b32(rr, 8 * (g + 128 + lane) + 4);
            Gn.head(w0, w1, G.ia + G.Lt, g + 64, nrec, in_b, lane);
            Gn.issue(in_b, lane, cw, sp);
        }
        const bool v = G.v;
        int lit = G.lit, mlx = G.mlx;
        const int Pm = G.Pm, o = G.o, anc = G.anc, ia = G.ia, Lt = G.Lt;
        const bool span = G.span;
        const int X0 = G.X0;
        int T;
        const int M = Pm - o;
        const int maxb = min(lit, M);
        if (v && maxb > 0) {   // catch-up (lz4.c:1017-1020): extend the match backwards while ip > anchor, match > start
            const uint32_t x = xp ^ xm;
            int bk = x ? (int)((uint32_t)__builtin_clz(x) >> 3) : 4;
            bk = min(bk, maxb);
            if (bk == 4) {                                   // (rare) past the first 4 bytes
                while (bk < maxb && in_b.b(Pm - 1 - bk) == in_b.b(M - 1 - bk)) bk++;
            }
            lit -= bk;
            mlx += bk;
        }
        const int S = v ? 3 + lit + lz4e::ext_len(lit) + lz4e::ext_len(mlx) : 0;
        const int pos = op + lz4e::wave_excl_scan(S, lane, T);
        const int litv = v ? lit : 0;
        const int litmax = (int)uni((uint32_t)lz4e::wave_max(litv));
        if (T <= lz4e::kRingB / 2 && litmax <= LZH_LZ4E_LITMAX && span) {
            const LDSA uint8_t* ib = (const LDSA uint8_t*)ibuf;
            const int ioff = ia + in_b.sh - X0 - ia;   // input position p lives at ib[p + ioff]
            // every lane writes its own sequence (lz4.c:1022-1135): token, one literal-length byte
            // when lit >= 15 (lit <= LZH_LZ4E_LITMAX <= 269 here), the literals (a lane-parallel copy as long as the
            // group's longest run), offset, match-length bytes
            if (op + T - R.flushed > lz4e::kRingB - 8) R.flush(op, false, lane);
            const int lx = lz4e::ext_len(lit), mx = lz4e::ext_len(mlx);
            const uint32_t token = ((uint32_t)min(lit, 15) << 4) | (uint32_t)min(mlx, 15);
            const int lp = pos + 1 + lx;
            if (v) {
                R.put(pos, token);
                if (lx) R.put(pos + 1, (uint32_t)(lit - 15));
            }
            for (int t = 0; t < litmax; t++)
                if (t < litv) R.put(lp + t, ib[anc + t + ioff]);
            const int mp = lp + lit;
            if (v) {
                R.put(mp, (uint32_t)o & 0xffu);
                R.put(mp + 1, (uint32_t)o >> 8);
            }
            for (int t = 0; ballot(v && t < mx); t++)
                if (v && t < mx) R.put(mp + 2 + t, t == mx - 1 ? (uint32_t)(mlx - 15) % 255u : 255u);
            op += T;
            if (op - R.flushed >= lz4e::kRingB / 2) R.flush(op, false, lane);
            wave_lds_fence();
        } else {
            for (int k = 0; k < 64 && g + k < nrec; k++) {
                const int kl = rdlanei(lit, k), km = rdlanei(mlx, k), ko = rdlanei(o, k), ka = rdlanei(anc, k);
                if (op + 256 - R.flushed > lz4e::kRingB) R.flush(op, false, lane);
                lz4e::put_seq_wave(R, in_b, op, ka, kl, ko, km, lane);
                op += 3 + kl + lz4e::ext_len(kl) + lz4e::ext_len(km);
            }
        }
        ia_end = ia + Lt;
    };
    for (int g = 0; g < nrec; g += 128) {
        step(GA, GB, g);
        if (g + 64 < nrec) step(GB, GA, g + 64);
    }
    const int ia = ia_end;
    // last literals (lz4.c:1204-1231): everything after the last match, the whole chunk if none
    const int last = n - ia;
    if (op + 256 - R.flushed > lz4e::kRingB) R.flush(op, false, lane);
    lz4e::put_seq_wave(R, in_b, op, ia, last, 0, -1, lane);
    op += 1 + last + lz4e::ext_len(last);
    R.flush(op, true, lane);
    if (lane == 0) csizes[chunk] = (uint32_t)op;
