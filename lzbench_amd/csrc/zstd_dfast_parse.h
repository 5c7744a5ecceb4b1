// lzbench_amd/csrc/zstd_dfast_parse.h -- zstd 1.5.2 double-fast: the level-3 parameters and the parse of one
// block, written once for the device kernel (zstdc_dfast_hip.hip) and for host code that wants the same walk.
//
// dfast_block restates ZSTD_compressBlock_doubleFast_noDict_generic (zstd_double_fast.c:51-253) position by
// position over an environment E that supplies the memory side:
//   E.r32(pos) / E.r64(pos)            little-endian reads of the frame at byte position pos
//   E.count_fwd(a, b, maxn)            equal bytes at a.. and b.., at most maxn (ZSTD_count)
//   E.count_bwd(a, b, maxn)            equal bytes going back from a-1 / b-1, at most maxn (the catch-up loops)
//   E.long_get / long_put, short_get / short_put   the two tables (entries: reference indexes, 0 = empty)
//   E.fence()                          table stores before it are visible to table loads after it
//   E.seq(lit_from, lit_len, offBase, mlen)        one stored sequence and its literals
// Every value the walk branches on is uniform over the callers of one E (a wave on the device).
// Positions are relative to the frame start; a reference index is position + 2 (ZSTD_window_init starts the
// window at index 2), which is what the tables hold, so "idx > prefixLowestIndex" reads as in the reference.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZDF_HD __host__ __device__
#else
#define ZDF_HD
#endif

namespace zdf {

struct DParams {
    int ok;
    uint32_t wlog, hlog, clog, mls, bsize;   // hlog: the long table (8-byte hashes); clog: the short one (mls bytes)
};

// ZSTD_getParams(3, n, 0) after ZSTD_adjustCParams_internal (zstd_compress.c:1316-1373); clevels.h:25-111 level 3
// is {W, C, H, S, minMatch, 0, ZSTD_dfast} in all four tables.  n == 0: unknown size, table 0 unadjusted.
ZDF_HD inline DParams params_for(int level, uint64_t n) {
    const uint8_t rows[4][4] = {{21, 16, 17, 5}, {18, 16, 16, 4}, {17, 15, 16, 5}, {14, 14, 15, 4}};
    DParams p{};
    if (level != 3) return p;
    const int unknown = n == 0;
    const int tid = unknown ? 0 : (n <= 262144) + (n <= 131072) + (n <= 16384);
    p.ok = 1;
    p.wlog = rows[tid][0];
    p.clog = rows[tid][1];
    p.hlog = rows[tid][2];
    p.mls = rows[tid][3];
    if (!unknown) {
        if (n < (1ull << 30)) {
            uint32_t srcLog = 6;                                   // ZSTD_HASHLOG_MIN
            if (n >= 64) { srcLog = 1; while ((1ull << srcLog) < n) srcLog++; }
            if (p.wlog > srcLog) p.wlog = srcLog;
        }
        if (p.hlog > p.wlog + 1) p.hlog = p.wlog + 1;
        if (p.clog > p.wlog) p.clog = p.wlog;                      // ZSTD_cycleLog(chainLog, dfast) = chainLog
    }
    if (p.wlog < 10) p.wlog = 10;                                  // ZSTD_WINDOWLOG_ABSOLUTEMIN
    uint64_t b = 1ull << p.wlog;
    if (b > 131072) b = 131072;
    if (n && b > n) b = n;
    p.bsize = (uint32_t)(b ? b : 1);
    return p;
}

ZDF_HD inline uint32_t hash8(uint64_t v, uint32_t hlog) { return (uint32_t)((v * 0xCF1BBCDCB7A56463ull) >> (64 - hlog)); }
ZDF_HD inline uint32_t hash_short(uint64_t v, uint32_t hlog, uint32_t mls) {
    return mls == 5 ? (uint32_t)(((v << 24) * 889523592379ull) >> (64 - hlog)) : ((uint32_t)v * 2654435761u) >> (32 - hlog);
}

// The parse of block [bs, be) of a frame; rep: the repcodes, in and out.  The literals after the last sequence
// ([return value, be)) are the caller's to store.
template <class Env>
ZDF_HD int dfast_block(Env& E, const DParams& P, int bs, int be, uint32_t rep[2]) {
    const int W = 1 << P.wlog;
    const int dl = bs > W ? bs - W : 0;                       // ZSTD_window_enforceMaxDist at the block start
    const int plow = (be - dl > W) ? be - W : dl;            // ZSTD_getLowestPrefixIndex(endIndex)
    const uint32_t plowIdx = (uint32_t)plow + 2;
    const int ilimit = be - 8;
    int ip = bs + (bs == plow);
    int anchor = bs;
    uint32_t off1 = rep[0], off2 = rep[1], saved = 0;
    {
        const int wlow = (ip - dl > W) ? ip - W : dl;
        const uint32_t maxRep = (uint32_t)(ip - wlow);
        if (off2 > maxRep) { saved = off2; off2 = 0; }
        if (off1 > maxRep) { saved = off1; off1 = 0; }
    }
    // the catch-up loop of the three match kinds: the match [ip, ..) from m grows backwards
    auto catch_up = [&](int& ipm, int m, uint32_t& mlen) {
        const int room = ipm - anchor < m - plow ? ipm - anchor : m - plow;
        const int back = room > 0 ? E.count_bwd(ipm, m, room) : 0;
        ipm -= back;
        mlen += (uint32_t)back;
    };
    for (;;) {                                                // one iteration per stored match
        int step = 1;
        int nextStep = ip + 256;                              // kStepIncr = 1 << kSearchStrength
        int ip1 = ip + step;
        if (ip1 > ilimit) break;
        uint32_t hl0 = hash8(E.r64(ip), P.hlog);
        uint32_t idxl0 = E.long_get(hl0);
        uint32_t curr = 0, hl1 = 0, mlen = 0, offset = 0;
        bool stored = false, found = false;
        do {                                                  // one iteration per searched position
            const uint64_t w0 = E.r64(ip), w1 = E.r64(ip1);
            const uint32_t hs0 = hash_short(w0, P.clog, P.mls);
            const uint32_t idxs0 = E.short_get(hs0);
            const bool rep_hit = off1 > 0 && E.r32(ip + 1 - (int)off1) == (uint32_t)(w0 >> 8);
            curr = (uint32_t)ip + 2;
            E.long_put(hl0, curr);
            E.short_put(hs0, curr);
            E.fence();
            if (rep_hit) {
                mlen = (uint32_t)E.count_fwd(ip + 5, ip + 5 - (int)off1, be - (ip + 5)) + 4;
                ip++;
                E.seq(anchor, ip - anchor, 1u, mlen);
                stored = true;
                break;
            }
            hl1 = hash8(w1, P.hlog);
            if (idxl0 > plowIdx && E.r64((int)idxl0 - 2) == w0) {                  // long match at ip
                const int m = (int)idxl0 - 2;
                mlen = (uint32_t)E.count_fwd(ip + 8, m + 8, be - (ip + 8)) + 8;
                offset = (uint32_t)(ip - m);
                catch_up(ip, m, mlen);
                found = true;
                break;
            }
            const uint32_t idxl1 = E.long_get(hl1);
            if (idxs0 > plowIdx && E.r32((int)idxs0 - 2) == (uint32_t)w0) {        // short match: _search_next_long
                if (idxl1 > plowIdx && E.r64((int)idxl1 - 2) == w1) {
                    const int m = (int)idxl1 - 2;
                    ip = ip1;
                    mlen = (uint32_t)E.count_fwd(ip + 8, m + 8, be - (ip + 8)) + 8;
                    offset = (uint32_t)(ip - m);
                    catch_up(ip, m, mlen);
                } else {
                    const int m = (int)idxs0 - 2;
                    mlen = (uint32_t)E.count_fwd(ip + 4, m + 4, be - (ip + 4)) + 4;
                    offset = (uint32_t)(ip - m);
                    catch_up(ip, m, mlen);
                }
                found = true;
                break;
            }
            if (ip1 >= nextStep) { step++; nextStep += 256; }
            ip = ip1;
            ip1 += step;
            hl0 = hl1;
            idxl0 = idxl1;
        } while (ip1 <= ilimit);
        if (!stored && !found) break;                         // _cleanup
        if (found) {                                          // _match_found
            off2 = off1;
            off1 = offset;
            if (step < 4) E.long_put(hl1, (uint32_t)ip1 + 2);
            E.seq(anchor, ip - anchor, offset + 3u, mlen);
        }
        ip += (int)mlen;                                      // _match_stored
        anchor = ip;
        if (ip <= ilimit) {
            const int c2 = (int)curr;                         // position of index curr + 2
            E.long_put(hash8(E.r64(c2), P.hlog), curr + 2);
            E.long_put(hash8(E.r64(ip - 2), P.hlog), (uint32_t)ip);
            E.short_put(hash_short(E.r64(c2), P.clog, P.mls), curr + 2);
            E.short_put(hash_short(E.r64(ip - 1), P.clog, P.mls), (uint32_t)ip + 1);
            while (ip <= ilimit && off2 > 0 && E.r32(ip) == E.r32(ip - (int)off2)) {   // immediate repcode
                const uint32_t rl = (uint32_t)E.count_fwd(ip + 4, ip + 4 - (int)off2, be - (ip + 4)) + 4;
                const uint32_t t = off2; off2 = off1; off1 = t;
                const uint64_t w = E.r64(ip);
                E.short_put(hash_short(w, P.clog, P.mls), (uint32_t)ip + 2);
                E.long_put(hash8(w, P.hlog), (uint32_t)ip + 2);
                E.seq(anchor, 0, 1u, rl);
                ip += (int)rl;
                anchor = ip;
            }
        }
        E.fence();
    }
    rep[0] = off1 ? off1 : saved;
    rep[1] = off2 ? off2 : saved;
    return anchor;
}

}  // namespace zdf
