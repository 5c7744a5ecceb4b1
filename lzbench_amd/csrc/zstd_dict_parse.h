// lzbench_amd/csrc/zstd_dict_parse.h -- zstd 1.5.2 fast strategy with a raw-content dictionary in a buffer of its
// own (ZSTD_compress_usingDict, include/lzbench_hip.h 3f): the parameters, the dictionary's table fill and the parse
// of a frame's one block, written once for the device kernels (zstd_dict_hip.hip) and for host code that wants the
// same walk (lzh_debug_zstd_dict_parse, the stand-alone census_dict_walk).
//
// Positions.  The reference gives the dictionary the indexes 2 .. 2 + D and the chunk 2 + D .. 2 + D + n
// (ZSTD_window_init starts at 2; ZSTD_window_update moves the dictionary to the extDict segment when the chunk is
// not contiguous with it), so prefixStartIndex = dictLimit = 2 + D and dictStartIndex = lowLimit = 2.  Table entries
// hold those indexes (0 = empty, below dictStartIndex).  The walk itself speaks in virtual positions relative to the
// chunk's first byte: p >= 0 is chunk byte p, p < 0 is dictionary byte D + p; index = p + 2 + D.
//
// ext_block restates ZSTD_compressBlock_fast_extDict_generic (zstd_fast.c:548-651) position by position over an
// environment E that supplies the memory side:
//   E.r32(p)                           little-endian 32 bits at virtual position p; p .. p + 3 lie in one segment
//   E.r64(p)                           64 bits at chunk position p >= 0
//   E.count_fwd(a, b, maxn)            equal bytes at chunk position a.. and virtual position b.., at most maxn; the
//                                      b side stays inside b's segment (ZSTD_count)
//   E.count_bwd(a, b, maxn)            equal bytes going back from a - 1 / b - 1, at most maxn, same rule
//   E.get(h) / E.put(h, idx)           the frame's table, a copy of the dictionary's filled table
//   E.fence()                          table stores before it are visible to table loads after it
//   E.seq(lit_from, lit_len, offBase, mlen)        one stored sequence and its literals
//   E.crossed()                        a forward count ran from the dictionary's end on into the chunk (zde::count2)
// The byte side of E -- r32, the counts, seq, crossed -- is zstd_dict_env.h's, for the host and for the device.
// Every value the walk branches on is uniform over the callers of one E (a wave on the device).
#pragma once
#include <stdint.h>

#include "zstd_dict_env.h"

namespace zdd {

constexpr uint32_t kDictMin = 8, kDictMax = 131072, kChunkMax = 131072;

struct XParams {
    int ok;
    uint32_t wlog, hlog, mls, tlen, bsize;
};

ZDE_HD inline bool level_ok(int level) { return level == 1 || (level <= -1 && level >= -5); }

// ZSTD_getParams_internal(level, n, D, ZSTD_cpm_noAttachDict) (zstd_compress.c:6272-6295, :1315-1373) for the levels
// whose row is ZSTD_fast in all four tables; clevels.h rows 0 and 1 as {W, H, minMatch, targetLength}.
// n + D <= 256 KiB here, so table 0 is never chosen.
ZDE_HD inline XParams params_for(int level, uint64_t n, uint64_t D) {
    const uint8_t rows[4][2][4] = {
        {{19, 13, 6, 1}, {19, 14, 7, 0}},
        {{18, 13, 5, 1}, {18, 14, 6, 0}},
        {{17, 12, 5, 1}, {17, 13, 6, 0}},
        {{14, 13, 5, 1}, {14, 15, 5, 0}},
    };
    XParams p{};
    if (!level_ok(level)) return p;
    const uint64_t t = n + D;
    const int tid = (t <= 262144) + (t <= 131072) + (t <= 16384);
    const int row = level < 0 ? 0 : 1;
    p.ok = 1;
    p.wlog = rows[tid][row][0];
    p.hlog = rows[tid][row][1];
    p.mls = rows[tid][row][2];
    p.tlen = level < 0 ? (uint32_t)(-level) : rows[tid][row][3];
    uint32_t srcLog = 6;                                          // ZSTD_HASHLOG_MIN
    if (t >= 64) { srcLog = 1; while ((1ull << srcLog) < t) srcLog++; }
    if (p.wlog > srcLog) p.wlog = srcLog;
    // ZSTD_dictAndWindowLog: the window already holds dictionary and source (2^wlog >= n + D), so it is wlog itself
    if (p.hlog > p.wlog + 1) p.hlog = p.wlog + 1;
    if (p.wlog < 10) p.wlog = 10;                                 // ZSTD_WINDOWLOG_ABSOLUTEMIN
    uint64_t b = 1ull << p.wlog;
    if (b > 131072) b = 131072;
    if (b > n) b = n;
    p.bsize = (uint32_t)(b ? b : 1);
    return p;
}

// ZSTD_hashPtr on the 8 bytes at a position
ZDE_HD inline uint32_t hashp(uint64_t v, uint32_t hlog, uint32_t mls) {
    switch (mls) {
        case 5: return (uint32_t)(((v << 24) * 889523592379ull) >> (64 - hlog));
        case 6: return (uint32_t)(((v << 16) * 227718039650203ull) >> (64 - hlog));
        case 7: return (uint32_t)(((v << 8) * 58295818150454627ull) >> (64 - hlog));
        default: return ((uint32_t)v * 2654435761u) >> (32 - hlog);
    }
}

// ZSTD_loadDictionaryContent + ZSTD_fillHashTable(ZSTD_dtlm_fast) (zstd_compress.c:4233-4253, zstd_fast.c:15-43): a
// dictionary of at most 8 bytes is referenced but not indexed; otherwise dictionary byte positions 0, 3, 6, .. below
// D - 9 are inserted, a later one replacing an earlier one: an entry is the largest inserted index of its bucket.
ZDE_HD inline uint32_t fill_count(uint64_t D) { return D <= 8 || D < 10 ? 0u : (uint32_t)((D - 10) / 3 + 1); }

// The (hashLog, minMatch) classes a batch can take: every n in 1 .. max_chunk with the dictionary of D bytes.
struct Classes {
    uint32_t count;
    uint32_t hlog[16], mls[16], off[16];   // off: the class's table in the table region, in bytes
    uint32_t bytes;                        // of all tables
};
ZDE_HD inline Classes classes_for(int level, uint64_t D, uint64_t max_chunk) {
    Classes C{};
    if (max_chunk < 1) max_chunk = 1;
    uint64_t n = 1;
    while (n <= max_chunk) {
        const XParams P = params_for(level, n, D);
        bool seen = false;
        for (uint32_t i = 0; i < C.count; i++) seen |= C.hlog[i] == P.hlog && C.mls[i] == P.mls;
        if (!seen && P.ok && C.count < 16) {
            C.hlog[C.count] = P.hlog;
            C.mls[C.count] = P.mls;
            C.off[C.count] = C.bytes;
            C.bytes += 4u << P.hlog;
            C.count++;
        }
        if (n == max_chunk) break;
        n = zde::next_class_n(n, D, max_chunk);
    }
    return C;
}
// every table of any batch fits this (level 1: hashLog 7 .. 15 below 16 KiB, then 13 and 14 with minMatch 6)
constexpr uint32_t kClassBytesMax = 4u * ((1u << 16) - (1u << 7)) + (4u << 13) + (4u << 14);

// The parse of the frame's block [0, n), 7 <= n <= 128 KiB, with a dictionary of D bytes.  The literals after the last
// sequence ([return value, n)) are the caller's to store.
template <class Env>
ZDE_HD int ext_block(Env& E, const XParams& P, uint32_t D, int n, uint32_t rep[2]) {
    const uint32_t psi = 2u + D;                              // prefixStartIndex; dictStartIndex = 2
    const int ilimit = n - 8;
    const int step0 = (int)(P.tlen + !P.tlen);
    int ip = 0, anchor = 0;
    uint32_t off1 = rep[0], off2 = rep[1];
    auto count2 = [&](int a, int m) { return zde::count2(E, a, m, n); };   // ZSTD_count_2segments
    while (ip < ilimit) {
        const uint32_t h = hashp(E.r64(ip), P.hlog, P.mls);
        const uint32_t midx = E.get(h);
        const uint32_t curr = (uint32_t)ip + psi;
        const uint32_t ridx = curr + 1 - off1;
        E.put(h, curr);
        E.fence();
        if ((psi - 1 - ridx >= 3u) && (off1 <= curr + 1 - 2u) &&
            E.r32((int)(ridx - psi)) == E.r32(ip + 1)) {
            const uint32_t rl = (uint32_t)count2(ip + 5, (int)(ridx - psi) + 4) + 4;
            ip++;
            E.seq(anchor, ip - anchor, 1u, rl);
            ip += (int)rl;
            anchor = ip;
        } else {
            const int m = (int)(midx - psi);
            if (midx < 2u || E.r32(m) != E.r32(ip)) {
                ip += ((ip - anchor) >> 8) + step0;           // kSearchStrength
                continue;
            }
            const int low = m < 0 ? -(int)D : 0;              // dictStart or prefixStart
            uint32_t ml = (uint32_t)count2(ip + 4, m + 4) + 4;
            const uint32_t offset = curr - midx;
            const int room = ip - anchor < m - low ? ip - anchor : m - low;
            const int back = room > 0 ? E.count_bwd(ip, m, room) : 0;   // catch up
            ip -= back;
            ml += (uint32_t)back;
            off2 = off1;
            off1 = offset;
            E.seq(anchor, ip - anchor, offset + 3u, ml);
            ip += (int)ml;
            anchor = ip;
        }
        if (ip <= ilimit) {
            const int c2 = (int)(curr - psi) + 2;
            E.put(hashp(E.r64(c2), P.hlog, P.mls), curr + 2);
            E.put(hashp(E.r64(ip - 2), P.hlog, P.mls), (uint32_t)(ip - 2) + psi);
            while (ip <= ilimit) {                            // immediate repcode
                const uint32_t cur2 = (uint32_t)ip + psi;
                const uint32_t ridx2 = cur2 - off2;
                if (!((psi - 1 - ridx2 >= 3u) && (off2 <= curr - 2u) && E.r32((int)(ridx2 - psi)) == E.r32(ip))) break;
                const uint32_t rl = (uint32_t)count2(ip + 4, (int)(ridx2 - psi) + 4) + 4;
                const uint32_t t = off2; off2 = off1; off1 = t;
                E.seq(anchor, 0, 1u, rl);
                E.put(hashp(E.r64(ip), P.hlog, P.mls), cur2);
                ip += (int)rl;
                anchor = ip;
            }
            E.fence();
        }
    }
    rep[0] = off1;
    rep[1] = off2;
    return anchor;
}

// A plain host environment: zde::HostBytes and a table of 1 << hlog entries.
struct HostEnv : zde::HostBytes {
    uint32_t* tab;
    uint32_t get(uint32_t h) const { return tab[h]; }
    void put(uint32_t h, uint32_t v) const { tab[h] = v; }
    void fence() const {}
};

// The host walk of one chunk: fills the table from the dictionary, parses; returns the number of sequences (the
// first `cap` are written to `seqs`), -1 for arguments outside the limits.  tab: 1 << 15 entries of scratch.
inline long host_walk(int level, const uint8_t* dict, uint64_t D, const uint8_t* src, uint64_t n, uint32_t* seqs,
                      uint64_t cap, uint32_t* tab) {
    if (!level_ok(level) || D < kDictMin || D > kDictMax || n > kChunkMax) return -1;
    if (n < 7) return 0;                                      // ZSTD_buildSeqStore: too small, no parse
    const XParams P = params_for(level, n, D);
    for (uint32_t i = 0; i < (1u << P.hlog); i++) tab[i] = 0;
    HostEnv E{{dict, (uint32_t)D, src, seqs, cap, 0, 0}, tab};
    const uint32_t nfill = fill_count(D);
    for (uint32_t q = 0; q < nfill; q++) {
        tab[hashp(E.r64((int)(3 * q) - (int)D), P.hlog, P.mls)] = 2u + 3u * q;
    }
    uint32_t rep[2] = {1u, 4u};
    ext_block(E, P, (uint32_t)D, (int)n, rep);
    return (long)E.ns;
}

}  // namespace zdd
