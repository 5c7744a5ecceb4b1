// lzbench_amd/csrc/zstd_dfast_dict_parse.h -- zstd 1.5.2 double-fast (level 3) with a raw-content dictionary in a
// buffer of its own (ZSTD_compress_usingDict, include/lzbench_hip.h 3h): the parameters, the dictionary's fill of the
// two tables and the parse of a frame's one block, written once for the device kernels (zstd_dfast_dict_hip.hip) and
// for host code that wants the same walk (lzh_debug_zstd_dfast_dict_parse, the stand-alone zstd_dfast_dict_walk).
//
// Positions are those of zstd_dict_parse.h: the dictionary has the indexes 2 .. 2 + D and the chunk 2 + D .. 2 + D + n,
// prefixStartIndex = dictLimit = 2 + D, dictStartIndex = lowLimit = 2; table entries hold those indexes (0 = empty).
// The walk speaks in virtual positions relative to the chunk's first byte: p >= 0 is chunk byte p, p < 0 is dictionary
// byte D + p; index = p + 2 + D.
//
// ext_block restates ZSTD_compressBlock_doubleFast_extDict_generic (zstd_double_fast.c:564-664) position by position
// over an environment E that supplies the memory side:
//   E.r32(p) / E.r64(p)                little-endian 32 / 64 bits at virtual position p, all inside one segment
//   E.count_fwd(a, b, maxn)            equal bytes at chunk position a.. and virtual position b.., at most maxn; the
//                                      b side stays inside b's segment (ZSTD_count)
//   E.count_bwd(a, b, maxn)            equal bytes going back from a - 1 / b - 1, at most maxn, same rule
//   E.long_get / long_put, short_get / short_put   the frame's two tables as the dictionary's fill left them
//   E.fence()                          table stores before it are visible to table loads after it
//   E.seq(lit_from, lit_len, offBase, mlen)        one stored sequence and its literals
//   E.event(k)                         branch k of the list below was reached (the host walk counts; the device ignores)
//   E.crossed()                        zde::count2 ran on into the chunk: the host walk's event kCrossed
// The byte side of E -- r32, r64 on the host, the counts, seq -- is zstd_dict_env.h's, shared with zstd_dict_parse.h.
// Every value the walk branches on is uniform over the callers of one E (a wave on the device).
#pragma once
#include <stdint.h>

#include "zstd_dfast_parse.h"
#include "zstd_dict_parse.h"

namespace zfd {

constexpr uint32_t kDictMin = zdd::kDictMin, kDictMax = zdd::kDictMax, kChunkMax = zdd::kChunkMax;

// the branches a walk can reach; "dict" / "chunk": where the match's source starts
enum Event : int {
    kRepDict = 0, kRepChunk,            // repcode at ip + 1
    kLongDict, kLongChunk,              // long match at ip
    kShortDict, kShortChunk,            // short match at ip kept (no long match at ip + 1)
    kLong1Dict, kLong1Chunk,            // short match at ip, long match at ip + 1 taken instead
    kRep2Dict, kRep2Chunk,              // one iteration of the offset_2 loop
    kCrossed,                           // a forward count ran from the dictionary's end on into the chunk's start
    kBackDictStart,                     // a catch-up stopped at the dictionary's first byte
    kBackChunkStart,                    // a catch-up stopped at the chunk's first byte
    kRepOverlap,                        // a repcode candidate refused by the three-byte overlap test
    kEvents
};

struct XParams {
    int ok;
    uint32_t wlog, hlog, clog, mls, bsize;   // hlog: the long table (8-byte hashes); clog: the short one (mls bytes)
};

ZDE_HD inline bool level_ok(int level) { return level == 3; }

// ZSTD_getParams_internal(3, n, D, ZSTD_cpm_noAttachDict) (zstd_compress.c:6272-6295, :1315-1373): the row is chosen
// by n + D and ZSTD_adjustCParams_internal runs on n + D -- window cut to srcLog, hashLog <= dictAndWindowLog + 1,
// chainLog <= dictAndWindowLog (ZSTD_cycleLog of dfast is chainLog), window floor 10 -- which is zdf::params_for of a
// source of n + D bytes: the window already holds dictionary and source (2^wlog >= n + D in every row n + D <= 256 KiB
// can choose), so ZSTD_dictAndWindowLog is wlog itself.  The block is the chunk.
ZDE_HD inline XParams params_for(int level, uint64_t n, uint64_t D) {
    XParams p{};
    if (!level_ok(level)) return p;
    const zdf::DParams R = zdf::params_for(3, n + D);
    p.ok = R.ok;
    p.wlog = R.wlog;
    p.hlog = R.hlog;
    p.clog = R.clog;
    p.mls = R.mls;
    uint64_t b = 1ull << p.wlog;
    if (b > 131072) b = 131072;
    if (b > n) b = n;
    p.bsize = (uint32_t)(b ? b : 1);
    return p;
}

// ZSTD_loadDictionaryContent + ZSTD_fillDoubleHashTable(ZSTD_dtlm_fast) (zstd_compress.c:4233-4256,
// zstd_double_fast.c:15-47; ZSTD_compress_usingDict reaches ZSTD_compressBegin_internal with ZSTD_dtlm_fast,
// zstd_compress.c:4704): with dtlm_fast the inner loop stops after i == 0, so dictionary byte positions 0, 3, 6, ..
// up to D - 10 go unconditionally into both tables (the short one under the mls hash, the long one under the 8-byte
// hash), a later one replacing an earlier one: an entry is the largest inserted index of its bucket.  The positions
// are zdd::fill_count(D) many.

// The (hashLog, chainLog, minMatch) classes a batch can take: every n in 1 .. max_chunk with the dictionary of D bytes.
struct Classes {
    uint32_t count;
    uint32_t hlog[16], clog[16], mls[16];
    uint32_t off[16];                      // the class's long table in the table region, in bytes; the short one follows
    uint32_t bytes;                        // of all tables
};
ZDE_HD inline Classes classes_for(int level, uint64_t D, uint64_t max_chunk) {
    Classes C{};
    if (max_chunk < 1) max_chunk = 1;
    uint64_t n = 1;
    while (n <= max_chunk) {
        const XParams P = params_for(level, n, D);
        bool seen = false;
        for (uint32_t i = 0; i < C.count; i++) seen |= C.hlog[i] == P.hlog && C.clog[i] == P.clog && C.mls[i] == P.mls;
        if (!seen && P.ok && C.count < 16) {
            C.hlog[C.count] = P.hlog;
            C.clog[C.count] = P.clog;
            C.mls[C.count] = P.mls;
            C.off[C.count] = C.bytes;
            C.bytes += (4u << P.hlog) + (4u << P.clog);
            C.count++;
        }
        if (n == max_chunk) break;
        n = zde::next_class_n(n, D, max_chunk);
    }
    return C;
}
// every pair of tables of any batch fits this: below 16 KiB hashLog = srcLog + 1 and chainLog = srcLog for srcLog
// 6 .. 14 (12 bytes << srcLog a pair), then {16, 15} up to 128 KiB and {16, 16} up to 256 KiB
constexpr uint32_t kClassBytesMax = 12u * ((1u << 15) - (1u << 6)) + (4u << 16) + (4u << 15) + (4u << 16) + (4u << 16);
constexpr uint32_t kClassCountMax = 11;

// The parse of the frame's block [0, n), 7 <= n <= 128 KiB, with a dictionary of D bytes.  The literals after the last
// sequence ([return value, n)) are the caller's to store.
// The reference's early return (zstd_double_fast.c:560, prefixStartIndex == dictStartIndex: the dictionary fell out of
// the window) cannot happen here: n + D never passes 2^windowLog (params_for), so lowLimit stays 2.
template <class Env>
ZDE_HD int ext_block(Env& E, const XParams& P, uint32_t D, int n, uint32_t rep[2]) {
    const uint32_t psi = 2u + D;                              // prefixStartIndex; dictStartIndex = 2
    const int ilimit = n - 8;
    int ip = 0, anchor = 0;
    uint32_t off1 = rep[0], off2 = rep[1];
    auto count2 = [&](int a, int m) { return zde::count2(E, a, m, n); };   // ZSTD_count_2segments (E.crossed: kCrossed)
    // the catch-up loop of the three match kinds: stops at dictStart for a source in the dictionary, else at prefixStart
    auto catch_up = [&](int& ipm, int m, uint32_t& mlen) {
        const int low = m < 0 ? -(int)D : 0;
        const int room = ipm - anchor < m - low ? ipm - anchor : m - low;
        const int back = room > 0 ? E.count_bwd(ipm, m, room) : 0;
        if (back > 0 && back == m - low) E.event(m < 0 ? kBackDictStart : kBackChunkStart);
        ipm -= back;
        mlen += (uint32_t)back;
    };
    while (ip < ilimit) {                                     // (< : ip + 1 is searched too)
        const uint64_t w0 = E.r64(ip);
        const uint32_t hs = zdf::hash_short(w0, P.clog, P.mls), hl = zdf::hash8(w0, P.hlog);
        const uint32_t midx = E.short_get(hs), lidx = E.long_get(hl);
        const uint32_t curr = (uint32_t)ip + psi;
        const uint32_t ridx = curr + 1 - off1;
        E.short_put(hs, curr);
        E.long_put(hl, curr);
        E.fence();
        uint32_t mlen;
        const bool rep_in = off1 <= curr + 1 - 2u, rep_clear = psi - 1 - ridx >= 3u;
        if (rep_in && !rep_clear) E.event(kRepOverlap);
        if (rep_clear && rep_in && E.r32((int)(ridx - psi)) == (uint32_t)(w0 >> 8)) {
            E.event(ridx < psi ? kRepDict : kRepChunk);
            mlen = (uint32_t)count2(ip + 5, (int)(ridx - psi) + 4) + 4;
            ip++;
            E.seq(anchor, ip - anchor, 1u, mlen);
        } else {
            uint32_t offset;
            if (lidx > 2u && E.r64((int)(lidx - psi)) == w0) {                      // long match at ip
                const int m = (int)(lidx - psi);
                E.event(m < 0 ? kLongDict : kLongChunk);
                mlen = (uint32_t)count2(ip + 8, m + 8) + 8;
                offset = curr - lidx;
                catch_up(ip, m, mlen);
            } else if (midx > 2u && E.r32((int)(midx - psi)) == (uint32_t)w0) {     // short match: long retry at ip + 1
                const uint64_t w1 = E.r64(ip + 1);
                const uint32_t h3 = zdf::hash8(w1, P.hlog);
                const uint32_t idx3 = E.long_get(h3);
                E.long_put(h3, curr + 1);
                if (idx3 > 2u && E.r64((int)(idx3 - psi)) == w1) {
                    const int m = (int)(idx3 - psi);
                    E.event(m < 0 ? kLong1Dict : kLong1Chunk);
                    mlen = (uint32_t)count2(ip + 9, m + 8) + 8;
                    ip++;
                    offset = curr + 1 - idx3;
                    catch_up(ip, m, mlen);
                } else {
                    const int m = (int)(midx - psi);
                    E.event(m < 0 ? kShortDict : kShortChunk);
                    mlen = (uint32_t)count2(ip + 4, m + 4) + 4;
                    offset = curr - midx;
                    catch_up(ip, m, mlen);
                }
            } else {
                ip += ((ip - anchor) >> 8) + 1;               // kSearchStrength
                continue;
            }
            off2 = off1;
            off1 = offset;
            E.seq(anchor, ip - anchor, offset + 3u, mlen);
        }
        ip += (int)mlen;
        anchor = ip;
        if (ip <= ilimit) {
            // the four complementary insertions
            const int c2 = (int)(curr - psi) + 2;
            const uint64_t wc = E.r64(c2);
            E.long_put(zdf::hash8(wc, P.hlog), curr + 2);
            E.long_put(zdf::hash8(E.r64(ip - 2), P.hlog), (uint32_t)(ip - 2) + psi);
            E.short_put(zdf::hash_short(wc, P.clog, P.mls), curr + 2);
            E.short_put(zdf::hash_short(E.r64(ip - 1), P.clog, P.mls), (uint32_t)(ip - 1) + psi);
            while (ip <= ilimit) {                            // immediate repcode
                const uint32_t cur2 = (uint32_t)ip + psi;
                const uint32_t ridx2 = cur2 - off2;
                const bool in2 = off2 <= cur2 - 2u, clear2 = psi - 1 - ridx2 >= 3u;
                if (in2 && !clear2) E.event(kRepOverlap);
                if (!(clear2 && in2 && E.r32((int)(ridx2 - psi)) == E.r32(ip))) break;
                E.event(ridx2 < psi ? kRep2Dict : kRep2Chunk);
                const uint32_t rl = (uint32_t)count2(ip + 4, (int)(ridx2 - psi) + 4) + 4;
                const uint32_t t = off2; off2 = off1; off1 = t;
                E.seq(anchor, 0, 1u, rl);
                const uint64_t w = E.r64(ip);
                E.short_put(zdf::hash_short(w, P.clog, P.mls), cur2);
                E.long_put(zdf::hash8(w, P.hlog), cur2);
                ip += (int)rl;
                anchor = ip;
            }
        }
        E.fence();
    }
    rep[0] = off1;
    rep[1] = off2;
    return anchor;
}

// A plain host environment: zde::HostBytes, a long table of 1 << hlog and a short table of 1 << clog entries, and the
// event counters.
struct HostEnv : zde::HostBytes {
    uint32_t* ltab;
    uint32_t* stab;
    uint64_t* events;   // kEvents counters, or null
    uint32_t long_get(uint32_t h) const { return ltab[h]; }
    uint32_t short_get(uint32_t h) const { return stab[h]; }
    void long_put(uint32_t h, uint32_t v) const { ltab[h] = v; }
    void short_put(uint32_t h, uint32_t v) const { stab[h] = v; }
    void fence() const {}
    void event(int k) const { if (events) events[k]++; }
    void crossed() const { event(kCrossed); }
};

// The host walk of one chunk: fills both tables from the dictionary, parses; returns the number of sequences (the
// first `cap` are written to `seqs`), -1 for arguments outside the limits.  tab: 2 << 16 entries of scratch; events:
// kEvents counters the walk adds to, or null.
inline long host_walk(int level, const uint8_t* dict, uint64_t D, const uint8_t* src, uint64_t n, uint32_t* seqs,
                      uint64_t cap, uint32_t* tab, uint64_t* events) {
    if (!level_ok(level) || D < kDictMin || D > kDictMax || n > kChunkMax) return -1;
    if (n < 7) return 0;                                      // ZSTD_buildSeqStore: too small, no parse
    const XParams P = params_for(level, n, D);
    uint32_t* ltab = tab;
    uint32_t* stab = tab + (1u << P.hlog);
    for (uint32_t i = 0; i < (1u << P.hlog) + (1u << P.clog); i++) tab[i] = 0;
    HostEnv E{{dict, (uint32_t)D, src, seqs, cap, 0, 0}, ltab, stab, events};
    const uint32_t nfill = zdd::fill_count(D);
    for (uint32_t q = 0; q < nfill; q++) {
        const uint64_t v = E.r64((int)(3 * q) - (int)D);
        stab[zdf::hash_short(v, P.clog, P.mls)] = 2u + 3u * q;
        ltab[zdf::hash8(v, P.hlog)] = 2u + 3u * q;
    }
    uint32_t rep[2] = {1u, 4u};
    ext_block(E, P, (uint32_t)D, (int)n, rep);
    return (long)E.ns;
}

}  // namespace zfd
