// lzbench_amd/csrc/zstdd_hufpar_body.inc -- body of the kernels that decode a long Huffman stream a wave
// (lzh_zstd_hufpar_kernel, decode_hip.hip; lzh_zstd_hufpar_ragged_kernel, zstd_ragged_split_hip.hip).  The
// including kernel has: out + (uint64_t)jf * chunk_size (the output address of frame jf, which the body reads from
// the job), chunk_size (converts to the largest frame of the launch: the per-frame temp is laid out for it), packed,
// packed_readable, offsets, status, zt, zst, jobs, njobs, par.
// A third consumer, lzh_zstd_hufpar_compact_kernel (zstd_ragged_split_compact_hip.hip), passes a zsplit::CompactBytes
// as chunk_size (a layout of stride 1 and no blocks) and a zsplit::HufTables as zt, whose operator+ takes the frame's
// index: the body must keep naming the table slots `zt + (uint64_t)jf * Z.stride + Z.hufs()` in that order, and use
// Z for nothing else, or that kernel reads another frame's tables.
// Textual, not a function: see zstdd_hdr_body.inc.
    using namespace zsplit;
    using namespace zstdd;
    __shared__ __attribute__((aligned(16))) uint32_t sbuf[kParCap / 4 + 128];   // dword d of the stream at d + 1
    __shared__ __attribute__((aligned(16))) uint16_t tab[2048];
    const int lane = threadIdx.x;
    const uint32_t jid = blockIdx.x >> 2, j = blockIdx.x & 3u;
    if (jid >= *njobs) return;
    const ZHuf* J = jobs + jid;
    const uint32_t jf = uni(J->frame), jns = uni(J->ns), jseg = uni(J->seg), jlast = uni(J->last);
    if (j >= jns) return;
    const int nsym = (int)(j == 3 ? jlast : jseg);
    const uint32_t sz = uni(J->sz[j]);
    if (!huf_par(par, nsym, sz) || uni((uint32_t)zst[jf]) != (uint32_t)kGo) return;
    const ZLayout Z = zlayout(chunk_size);
    const int tl = (int)uni(J->tl);
    {   // the section's table (2^11 16-bit cells: symbol | nbBits << 8)
        const uint32_t* tb = (const uint32_t*)(zt + (uint64_t)jf * Z.stride + Z.hufs() + (uint64_t)uni(J->tblk) * kHufSlot);
        for (int i = lane; i < 1024; i += LZH_WAVE) ((LDSA uint32_t*)tab)[i] = tb[i];
    }
    // the stream's bytes [A, A + X] (A 4-aligned, the stream starting at byte x0), bits below its start zero
    const int64_t s0 = (int64_t)offsets[jf] + (int64_t)uni(J->s0[j]);
    const int64_t A = s0 & ~3ll;
    const int x0 = (int)(s0 & 3), X = x0 + (int)sz - 1;
    const int lo = 8 * x0;
    const int nd = (X + 4) >> 2;
    const int64_t avail = (int64_t)packed_readable - A;
    const rsrc_t r = make_rsrc(packed + A, (uint32_t)max<int64_t>(0, min<int64_t>(avail, (int64_t)nd * 4)));
    {
        if (lane == 0) sbuf[0] = 0u;
        // (LDS-DMA rows of 64 dwords, one wait; past nd the range check reads zeros)
        for (int d0 = 0; d0 < nd + 2; d0 += LZH_WAVE)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)(sbuf + 1 + d0), 4,
                                                     4 * (d0 + lane), 0, 0, 0);
    }
    wait_vm();
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): table and stream in LDS
    const uint32_t lastb = (sbuf[(X >> 2) + 1] >> (8 * (X & 3))) & 0xffu;
    // bits [bq, bq + tl) (bq >= -32: the zero dword below the stream), zero below lo
    auto bits = [&](int bq) -> uint32_t {
        const int b = bq + 32, d = b >> 5;
        const volatile LDSA uint32_t* s = (const volatile LDSA uint32_t*)sbuf;
        uint32_t v = __builtin_amdgcn_ubfe(__builtin_amdgcn_alignbit(s[d + 1], s[d], (uint32_t)b & 31u), 0u, (uint32_t)tl);
        if (bq < lo) v &= lo - bq >= 32 ? 0u : (~0u << (lo - bq));
        return v;
    };
    const int P0 = 8 * X + (lastb ? hb32(lastb) : 0);   // (the end mark: checked non-zero by the header kernel)
    // this lane's share (P0 - lane * seg, P0 - (lane + 1) * seg], the last one down to lo
    const int nbits = P0 - lo;
    const int seg = (nbits + LZH_WAVE - 1) / LZH_WAVE;
    const int top = P0 - lane * seg;
    const int bot = lane == LZH_WAVE - 1 ? lo : max(P0 - (lane + 1) * seg, lo);
    const int guard = seg + 64;
    // decode the share from start: the chain's exit (the first symbol top at or below bot) and its symbols
    auto pass = [&](bool act, int start, int& ex, int& cnt, uint8_t* wdst) {
        int P = start, c = 0;
        for (int it = 0; it < guard; it++) {
            const bool go = act && P > bot;
            if (!ballot(go)) break;
            if (go) {
                const uint32_t e = ((const volatile LDSA uint16_t*)tab)[bits(P - tl)];
                if (wdst) wdst[c] = (uint8_t)e;
                P -= (int)(e >> 8);
                c++;
            }
        }
        if (act) { ex = P; cnt = c; }
    };
    int start = lane == 0 ? P0 : top, ex = 0, cnt = 0;
    pass(true, start, ex, cnt, nullptr);
    for (int round = 0; round < LZH_WAVE; round++) {   // until every share starts where the previous one ends
        const int prev = (int)lane_gather((uint32_t)ex, lane > 0 ? lane - 1 : 0);
        const int want = lane == 0 ? P0 : prev;
        const bool ch = want != start;
        if (!ballot(ch)) break;
        // decode from the new start (A) alongside the chain already counted from the old one (B), always the
        // higher of the two, until they meet -- the rest is the counted chain -- or A leaves the share
        int PA = want, cA = 0, PB = start, cB = 0;
        bool met = false;
        for (int it = 0; it < 2 * guard; it++) {
            met = met || (ch && PA == PB);
            const bool go = ch && !met && PA > bot;
            if (!ballot(go)) break;
            if (go) {
                const bool a = PA > PB;
                const uint32_t e = ((const volatile LDSA uint16_t*)tab)[bits((a ? PA : PB) - tl)];
                const int nb = (int)(e >> 8);
                PA -= a ? nb : 0;
                cA += a ? 1 : 0;
                PB -= a ? 0 : nb;
                cB += a ? 0 : 1;
            }
        }
        if (ch) {
            if (met) {
                cnt = cA + (cnt - cB);   // (ex: the counted chain's exit)
            } else {
                ex = PA;
                cnt = cA;
            }
            start = want;
        }
    }
    const int incl = groups::wave_incl_scan(cnt);
    const int total = rdlanei(incl, LZH_WAVE - 1);
    const bool exact = total == nsym && rdlanei(ex, LZH_WAVE - 1) == lo;
    if (exact) {
        uint8_t* dst = out + (uint64_t)jf * chunk_size + uni(J->dst) + (uint64_t)j * jseg + (incl - cnt);
        int ex2 = 0, cnt2 = 0;
        pass(true, start, ex2, cnt2, dst);
    } else if (lane == 0) {   // not consumed exactly: X2's verdict (the one-wave decoder) or corrupt
        if (uni(J->x2)) {
            atomicMax(&zst[jf], kLegacy);
        } else if (atomicMax(&zst[jf], kDone) != kDone) {
            status[jf] = ZC;
        }
    }
