// lzbench_amd/csrc/zstdd_seq_body.inc -- body of the zstd split decoder's sequence kernels (lzh_zstd_seq_kernel,
// decode_hip.hip; lzh_zstd_seq_compact_kernel, zstd_ragged_split_compact_hip.hip) after the frame lookup.  The including
// kernel has: S (its LDS), lane, f and live (per lane: the lane's frame, and whether it has one at kGo), Z (the layout
// of the lane's frame's area), zb (that area; a lane without a frame parks on one it never touches), zt + (uint64_t)nchunks *
// Z.stride (the waves' dummy words), which and gridDim (the second launch of a planned pair takes the words' upper half), packed,
// packed_readable, offsets, zfr, stats.
// Textual, not a function: see zstdd_hdr_body.inc.
    const ZBlk* blk = (const ZBlk*)zb;
    ZExe* ex = (ZExe*)(zb + Z.exe());
    uint64_t* seqs = (uint64_t*)(zb + Z.seqs());
    int nblk = 0, n = 0;
    int64_t ioff = 0;
    if (live) {
        const ZFrame fr = zfr[f];
        nblk = fr.nblk;
        n = fr.n;
        ioff = (int64_t)offsets[f];
    }
    // (fills are global_load_lds rows from per-lane addresses: with a buffer resource the kernel's
    // scalar-register pressure moved it to vector registers and every fill became a waterfall loop)
    const int64_t readable = (int64_t)packed_readable;
    uint64_t* const dummy = (uint64_t*)(zt + (uint64_t)nchunks * Z.stride) +
                            64ull * (blockIdx.x + (which == 1 ? gridDim.x : 0u));   // (the wave's slice)
    const int lo4 = lane * 4;
    int phase = live ? 0 : 3, res = kGo;   // 0 block start, 1 waiting for fills, 2 sequences, 3 finished
    int b = 0, op = 0, rep0 = 1, rep1 = 4, rep2 = 8;
    uint32_t sfl = 0;                                           // sequences stored
    int rs = 0, lp = 0, nseq = 0, i = 0, lA = 0, oA = 0, mA = 0;
    uint32_t sLL = 0, sOF = 0, sML = 0;
    const uint8_t *tLL = zb, *tOF = zb, *tML = zb;   // the block's table slots
    int64_t A = 0;                       // the stream's first byte rounded down to a dword (absolute)
    int P = 0, lo = 0;                   // bits [lo, P) of the stream are unread (positions from A)
    int hb0 = 0, hb1 = 0;                // the 32-dword stream blocks in ring halves 0 / 1
    int rdy = 0, req = 0, iss = 0;       // halves ready / requested / in flight (bits 0, 1)
    int lowok = 1 << 30;                 // a step runs while P >= lowok
    bool treq = false, tiss = false, trdy = false;
    const int smax = (int)Z.smax;

    // bits [q, q + w) of the stream (w <= 31): rows of dwords q / 32 and the one above, a funnel
    // shift and a bit-field extract
    auto fld = [&](int q, int w) -> uint32_t {
        const LDSA uint8_t* a = S + kLdsRing + ((q >> 5) & 63) * kRow + lo4;
        const uint32_t v = __builtin_amdgcn_alignbit(*(const LDSA uint32_t*)(a + kRow), *(const LDSA uint32_t*)a,
                                                     (uint32_t)q & 31u);
        return __builtin_amdgcn_ubfe(v, 0u, (uint32_t)w);
    };

    // every step stores one record per lane at seqp[sfl] and advances sfl when the record is kept: a lane
    // without one writes the slot its next record overwrites (or the spare slot past its last), a lane
    // without a frame its own word of the wave's dummy slice (its sfl stays 0)
    uint64_t* const seqp = live ? seqs : dummy + lane;
    // (the lane's column of the bit ring, opaque to the compiler: it would split the ring's offset back out
    // and add it per address, the ds_read2 offset field being too small for it)
    const LDSA uint8_t* rb = S + kLdsRing + lo4;
    asm volatile("" : "+v"(rb));
    uint64_t sst[6] = {0, 0, 0, 0, 0, 0}, tmark = 0;   // (LZH_ZSTD_STATS: uniform points, steps, ...)
    const uint64_t tm0 = LZH_ZSTD_STATS ? __builtin_amdgcn_s_memtime() : 0, tr0 = LZH_ZSTD_STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the compiler's own wait tracking sees it
    for (int ival = 0;; ival++) {
        if (LZH_ZSTD_STATS) {
            const uint64_t t = __builtin_amdgcn_s_memtime();
            if (ival) sst[1] += t - tmark;
            tmark = t;
            sst[2]++;
        }
        // ---- uniform point
        // every memory operation but the previous point's kSB flush stores (issued after its fills) is done
        __builtin_amdgcn_s_waitcnt(vmcnt_imm(kSB));
        if (LZH_ZSTD_STATS) sst[5] += __builtin_amdgcn_s_memtime() - tmark;
        rdy |= iss;
        iss = 0;
        if (tiss) { tiss = false; trdy = true; }
        if (phase == 1 && trdy && rdy == 3) {   // the block's first states (LL, OF, ML)
            sLL = fld(P - lA, lA);
            sOF = fld(P - lA - oA, oA);
            sML = fld(P - lA - oA - mA, mA);
            P -= lA + oA + mA;
            phase = 2;
        }
        if (LZH_ZSTD_STATS) sst[3] += ballot(phase == 0) != 0;
        while (phase == 0) {   // the next blocks, up to one with sequences (or the end of the frame)
            if (b == nblk) {
                if (op != n) res = ZC;
                phase = 3;
                break;
            }
            const ZBlk B = blk[b];
            const int si = sfl;
            if (B.type != 2) {
                if ((int)B.size > n - op) { res = ZC; phase = 3; break; }
                ex[b] = ZExe{(uint32_t)op, (uint32_t)si};
                op += (int)B.size;
                b++;
                continue;
            }
            rs = (int)B.rs;
            if (B.ltype != 0 && rs > n - op) { res = ZC; phase = 3; break; }
            ex[b] = ZExe{(uint32_t)op, (uint32_t)si};
            lp = 0;
            i = 0;
            nseq = (int)B.nseq;
            b++;
            if (nseq == 0) {
                if (rs > n - op) { res = ZC; phase = 3; break; }
                op += rs;
                continue;
            }
            if ((int)sfl + nseq > smax - 1) { res = kLegacy; phase = 3; break; }   // (the layout's record slots, one spare)
            lA = (int)(B.logs & 255u);
            oA = (int)((B.logs >> 8) & 255u);
            mA = (int)(B.logs >> 16);
            const uint8_t* cz = zb + Z.cells();
            tLL = cz + (size_t)B.tll * kSlot;
            tML = cz + (size_t)B.tml * kSlot + 2048;
            tOF = cz + (size_t)B.tof * kSlot + 4096;
            treq = true;
            trdy = false;
            // the stream's end mark (BIT_initDStream) and the two blocks below it
            const int64_t s0 = ioff + (int64_t)B.pos;
            const int size = (int)B.size;
            if (size <= 0) { res = ZC; phase = 3; break; }
            A = s0 & ~3ll;
            const int x0 = (int)(s0 & 3), X = x0 + size - 1;
            const uint32_t last = packed[A + X];
            if (last == 0) { res = ZC; phase = 3; break; }
            lo = 8 * x0;
            P = 8 * X + hb32(last);
            const int bt = (P - 1) >> 10;
            hb0 = (bt & 1) ? bt - 1 : bt;
            hb1 = (bt & 1) ? bt : bt - 1;
            rdy = 0;
            iss = 0;
            req = 3;
            phase = 1;
        }
        if (phase == 2) {   // the upper block, once the reader is below it, takes the block under the lower one
            const int top = (P - 1) >> 10;
            const bool r0 = (rdy & 1) != 0 && hb0 > top && hb0 > hb1, r1 = (rdy & 2) != 0 && hb1 > top && hb1 > hb0;
            if (r0) { hb0 = hb1 - 1; rdy &= ~1; req |= 1; }
            if (r1) { hb1 = hb0 - 1; rdy &= ~2; req |= 2; }
        }
        if (ballot(treq)) {
            if (treq) {
#pragma unroll 8
                for (int r = 0; r < 512; r++) dma_row(tLL + 4 * r, S + r * kRow);
#pragma unroll 8
                for (int r = 0; r < 512; r++) dma_row(tML + 4 * r, S + kLdsML + r * kRow);
#pragma unroll 8
                for (int r = 0; r < 128; r++) dma_row(tOF + 4 * r, S + kLdsOF + r * kRow);
                treq = false;
                tiss = true;
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (ballot(req & (1 << h))) {
                const int64_t x0 = A + 128ll * (h ? hb1 : hb0);
                // a block wholly outside the packed bytes holds no stream data: any readable bytes will do
                const bool part = x0 >= 0 && x0 < readable && x0 + 128 > readable;
                const uint8_t* g = packed + (x0 < 0 || x0 >= readable ? 0 : x0);
                if ((req & (1 << h)) && !part) {
#pragma unroll
                    for (int k = 0; k < 32; k++) dma_row(g + 4 * k, S + kLdsRing + (h * 32 + k) * kRow);
                    if (h == 0) dma_row(g, S + kLdsRing + 64 * kRow);   // (the mirror of row 0)
                }
                if (ballot((req & (1 << h)) && part)) {   // (the packed bytes end inside the block)
                    if ((req & (1 << h)) && part) {
                        for (int k = 0; k < 32; k++)
                            dma_row(packed + (x0 + 4 * k < readable - 4 ? x0 + 4 * k : ((readable - 4) & ~3ll)), S + kLdsRing + (h * 32 + k) * kRow);
                        if (h == 0) dma_row(packed + x0, S + kLdsRing + 64 * kRow);
                    }
                }
                if (req & (1 << h)) {
                    req &= ~(1 << h);
                    iss |= 1 << h;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // the lowest position a step may start from: the ready blocks below the reader + 90 bits
        lowok = (rdy == 3 ? 1024 * min(hb0, hb1) : (rdy == 1 ? 1024 * hb0 : (rdy == 2 ? 1024 * hb1 : (1 << 30)))) + 90;
        if (phase != 2) lowok = 1 << 30;
        if (LZH_ZSTD_STATS) {
            const uint64_t t = __builtin_amdgcn_s_memtime();
            sst[0] += t - tmark;
            tmark = t;
        }
        if (!ballot(phase != 3)) break;
        if (ival > (smax + 64 * (int)Z.bmax) / 2) {   // (a bound every lane meets: a stuck lane's frame goes to
            if (phase != 3) { res = kLegacy; phase = 3; }   // the one-wave decoder)
            lowok = 1 << 30;
        }
        // the cells of the states (read one step ahead from here on: a step reads the next step's cells
        // as soon as its states are known, under its checks and record)
        uint32_t cL = 0, cM = 0, cO = 0;
        if (phase == 2) {
            cL = *(const LDSA uint32_t*)(S + sLL * kRow + lo4);
            cM = *(const LDSA uint32_t*)(S + kLdsML + sML * kRow + lo4);
            cO = *(const LDSA uint16_t*)(S + kLdsOF + (sOF >> 1) * kRow + lo4 + (sOF & 1) * 2);
        }
        // ---- kSB steps: each stores exactly one record per lane (a dummy word for a lane without one),
        // so that the next point's vmcnt(kSB) waits for this point's fills and not for these stores
        for (int k = 0; k < kSB; k++) {
            const bool act = P >= lowok;
            uint32_t r0 = 0, r1 = 0;
            bool keep = false;
            if (act) {
                const uint32_t eL = cL, eM = cM, eO = cO;
                const int ofc = (int)(eO >> 9);
                const uint32_t eOx = eO & 511u;
                const int no = (int)__builtin_ctz(eOx);
                const int am = (int)__builtin_amdgcn_ubfe(eM, 13u, 5u), al = (int)__builtin_amdgcn_ubfe(eL, 13u, 5u);
                const int nl = (int)__builtin_amdgcn_ubfe(eL, 9u, 4u), nm = (int)__builtin_amdgcn_ubfe(eM, 9u, 4u);
                const int ns = nl + nm + no;
                const bool lastq = i + 1 == nseq;
                // the fields: offset extra bits, ML extra bits, LL extra bits, LL / ML / OF state bits
                const int P1 = P - ofc, P2 = P1 - am, P3 = P2 - al, P4 = P3 - (lastq ? 0 : ns);
                // (the eight ring loads issued together, then used: the scheduler would wait after each pair)
                const LDSA uint8_t* a1 = rb + ((P1 >> 5) & 63) * kRow;
                const LDSA uint8_t* a2 = rb + ((P2 >> 5) & 63) * kRow;
                const LDSA uint8_t* a3 = rb + ((P3 >> 5) & 63) * kRow;
                const LDSA uint8_t* a4 = rb + ((P4 >> 5) & 63) * kRow;
                const uint32_t w1l = *(const LDSA uint32_t*)a1, w1h = *(const LDSA uint32_t*)(a1 + kRow);
                const uint32_t w2l = *(const LDSA uint32_t*)a2, w2h = *(const LDSA uint32_t*)(a2 + kRow);
                const uint32_t w3l = *(const LDSA uint32_t*)a3, w3h = *(const LDSA uint32_t*)(a3 + kRow);
                const uint32_t w4l = *(const LDSA uint32_t*)a4, w4h = *(const LDSA uint32_t*)(a4 + kRow);
                __builtin_amdgcn_sched_barrier(0);
                const uint32_t ob = __builtin_amdgcn_ubfe(__builtin_amdgcn_alignbit(w1h, w1l, (uint32_t)P1 & 31u), 0u, (uint32_t)ofc);
                const uint32_t mb = __builtin_amdgcn_ubfe(__builtin_amdgcn_alignbit(w2h, w2l, (uint32_t)P2 & 31u), 0u, (uint32_t)am);
                const uint32_t lb = __builtin_amdgcn_ubfe(__builtin_amdgcn_alignbit(w3h, w3l, (uint32_t)P3 & 31u), 0u, (uint32_t)al);
                const uint32_t sb = __builtin_amdgcn_ubfe(__builtin_amdgcn_alignbit(w4h, w4l, (uint32_t)P4 & 31u), 0u,
                                                          (uint32_t)(lastq ? 0 : ns));
                const int ml = (int)((__builtin_amdgcn_ubfe(eM, 18u, 1u) << am) + (eM >> 19) + mb);
                const int ll = (int)((__builtin_amdgcn_ubfe(eL, 18u, 1u) << al) + (eL >> 19) + lb);
                // repcodes (ZSTD_decodeSequence): ofc > 1 a new offset; else repcode j = ofc + ll0 + bit
                // (selects on lane masks: the compiler would branch on them)
                const bool big = ofc > 1;
                const int j = ofc + (int)((eL >> 18) == 0) + (int)ob;
                int t = vsel(j == 0, rep0, vsel(j == 1, rep1, vsel(j == 2, rep2, rep0 - 1)));
                t += t == 0;
                const int off = vsel(big, (int)((1u << ofc) - 3u + ob), t);
                const int nrep1 = vsel(big | (j >= 1), rep0, rep1);
                rep2 = vsel(big | (j >= 2), rep1, rep2);
                rep1 = nrep1;
                rep0 = off;
                sLL = (eL & 511u) + (sb >> (nm + no));
                sML = (eM & 511u) + __builtin_amdgcn_ubfe(sb, (uint32_t)no, (uint32_t)nm);
                sOF = ((eOx - (1u << no)) >> 1) + __builtin_amdgcn_ubfe(sb, 0u, (uint32_t)no);
                P = P4;
                cL = *(const LDSA uint32_t*)(S + sLL * kRow + lo4);
                cM = *(const LDSA uint32_t*)(S + kLdsML + sML * kRow + lo4);
                cO = *(const LDSA uint16_t*)(S + kLdsOF + (sOF >> 1) * kRow + lo4 + (sOF & 1) * 2);
                // the checks of ZSTD_execSequence and the layout's limit (else the one-wave decoder decodes).
                // Per step only the offset and the record width: the stream position only falls and the
                // literals used / the output plus the literals left only grow, so the checks on those hold
                // at every sequence of a block exactly when they hold at its last -- that is where they are
                // made (with the reference's end of stream: it updates the states after the last sequence too
                // and accepts an exhausted or overrun stream there, ZSTD_decompressSequences_body: reload >=
                // completed).  A frame that fails is not executed, so nothing reads the records before it.
                const bool bad = (uint32_t)off > (uint32_t)(op + ll);
                // (the output bound per step too: op and lp are 32-bit, and up to 2^15 sequences of < 2^18 bytes
                // each could wrap op back into range before the block-end check; such a frame goes to the one-wave
                // decoder, whose verdict is ZSTD_execSequence's.  With it op <= n at every step, so lp <= op never
                // wraps either.)
                const bool lim17 = ((ll | ml) >= (1 << kLenBits)) | (op + ll + ml > n);
                r0 = (uint32_t)ll | ((uint32_t)ml << kLenBits);
                r1 = ((uint32_t)ml >> (32 - kLenBits)) | ((uint32_t)off << (2 * kLenBits - 32));
                keep = !(bad | lim17);
                lp += ll;
                op += ll + ml;
                i++;
                if (bad | lim17 | lastq) {   // an error, a limit, or the block's end (its last literals)
                    const int rem = rs - lp;
                    if (bad | lim17) {
                        res = bad ? ZC : kLegacy;
                        phase = 3;
                    } else if ((P < lo) | (P - lo > ns) | (rem < 0) | (rem > n - op)) {
                        res = ZC;
                        phase = 3;
                    } else {
                        op += rem;
                        phase = 0;
                    }
                    lowok = 1 << 30;
                }
                if (LZH_ZSTD_STATS) sst[4]++;
            }
            seqp[sfl] = (uint64_t)r0 | ((uint64_t)r1 << 32);
            sfl += keep;
        }
    }
    if (LZH_ZSTD_STATS && stats && lane == 0) {
        for (int k = 0; k < 6; k++) atomicAdd(&stats[k], (unsigned long long)sst[k]);
        atomicAdd(&stats[8], (unsigned long long)(__builtin_amdgcn_s_memtime() - tm0));   // (the in-kernel clock)
        atomicAdd(&stats[9], (unsigned long long)(__builtin_amdgcn_s_memrealtime() - tr0));
    }
    if (LZH_ZSTD_STATS && stats && live && res == kLegacy) atomicAdd(&stats[6], 1ull);
    if (live) zfr[f].sv = res;   // (kGo, kLegacy or an error: lzh_zstd_exec_kernel applies it)
