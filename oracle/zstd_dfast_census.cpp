// oracle/zstd_dfast_census.cpp -- the zstd level-3 (double-fast) parse on the host, with a census of its events
// (TEST INFRASTRUCTURE ONLY).  It instantiates zdf::dfast_block (lzbench_amd/csrc/zstd_dfast_parse.h, the walk the
// match kernel runs) over plain memory and two std::vector tables, walks a frame block by block as
// zstdc_dfast_match_body.inc does (params_for(3, n), tables zeroed per frame and kept across blocks, repcodes
// carried between blocks and confirmed as the entropy stage confirms them), returns the stored sequences and counts
// the classes tests/zstd_dfast_census.py documents.
//
// The header is not changed: every counter lives in HostEnv and in the wrapper around each dfast_block call.  The
// environment sees the walk as a sequence of calls and follows it with a small state machine:
//   long_put(v), short_put(v), fence  -- in that order and with one value -- is the search's store of position v - 2;
//   the count_fwd after it names the match kind by its first argument (ip + 5: repcode at ip + 1, ip + 8: long at
//   ip, ip + 4: short kept, ip1 + 8: long at ip + 1); a long_put between that and seq is the hl1 insertion; puts
//   after seq are the post-match insertions; a count_fwd after seq is an immediate repcode.
// At a search's fence the environment also works out by itself what the walk must do next (from the table values it
// handed out and its own reads); a walk that does something else is counted as invariant/model-mismatch, which the
// tests require to be 0, like the other invariant/ classes.
//
// Build: oracle/Makefile (libzdfcensus.so); with -DZDF_CENSUS_MAIN a stand-alone program that walks the files named
// on its command line, for a sanitizer build.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../lzbench_amd/csrc/zstd_dfast_parse.h"

namespace {

#define ZDF_CLASSES(X)                                                                                               \
    X(ROW0, "params/row/n>262144") X(ROW1, "params/row/n<=262144") X(ROW2, "params/row/n<=131072")                    \
    X(ROW3, "params/row/n<=16384") X(MLS4, "params/mls4") X(MLS5, "params/mls5") X(WLOG_CL, "params/wlog-clamped")    \
    X(HLOG_CL, "params/hlog-clamped") X(CLOG_CL, "params/clog-clamped") X(WLOG_10, "params/wlog-raised-to-10")        \
    X(BLOCKS1, "frame/blocks/1") X(BLOCKS2, "frame/blocks/2") X(BLOCKS3, "frame/blocks/3+")                           \
    X(B_FIRST, "block/first") X(B_LATER, "block/later") X(B_RAW, "block/under-7-bytes")                               \
    X(B_SHORT, "block/too-short-to-search") X(B_DL, "block/dl>0") X(B_PLOW, "block/plow>dl")                          \
    X(B_OFF1, "block/off1-saved") X(B_OFF2, "block/off2-saved") X(B_SAVED_LATER, "block/rep-saved-on-later-block")    \
    X(B_RESTORED, "block/saved-restored") X(B_UNCONF, "block/repcodes-unconfirmed")                                   \
    X(S_REP, "search/rep-hit") X(S_LONG, "search/long-hit") X(S_SHORT, "search/short-kept")                           \
    X(S_LONG1, "search/long-at-ip+1") X(S_OUT, "search/ran-out") X(S_ENDMATCH, "search/ends-at-match")                \
    X(STEP1, "step/1") X(STEP2, "step/2") X(STEP3, "step/3") X(STEP4, "step/4+")                                      \
    X(HL1_IN, "post/hl1-inserted") X(HL1_SKIP, "post/hl1-skipped")                                                    \
    X(RL_EMPTY, "reject/long/empty") X(RL_STALE, "reject/long/stale") X(RL_COLL, "reject/long/collision")             \
    X(RS_EMPTY, "reject/short/empty") X(RS_STALE, "reject/short/stale") X(RS_COLL, "reject/short/collision")          \
    X(FRESH_L, "hit/fresh-long") X(FRESH_S, "hit/fresh-short")                                                        \
    X(CU0, "catchup/0") X(CU1, "catchup/1-63") X(CU64, "catchup/64") X(CU65, "catchup/65+")                           \
    X(CU_ANCHOR, "catchup/to-anchor") X(CU_PLOW, "catchup/to-plow")                                                   \
    X(CF0, "count/0") X(CF1, "count/1-255") X(CF256, "count/256") X(CF257, "count/257-511") X(CF512, "count/512+")    \
    X(CF_END, "count/to-block-end") X(ML_LONG, "ml/>=65539") X(ML_LONG_REP, "ml/>=65539-rep")                         \
    X(LIT0, "lit/0") X(LIT1, "lit/1-63") X(LIT64, "lit/64") X(LIT65, "lit/65-255") X(LIT256, "lit/256")               \
    X(LIT257, "lit/>256") X(LIT_LONG, "lit/>=65536")                                                                  \
    X(OFF1, "off/1") X(OFF2, "off/2-7") X(OFF64K, "off/>=65536") X(OFF_EARLIER, "off/earlier-block")                  \
    X(OFF_W, "off/window")                                                                                            \
    X(INS_DONE, "post/insert-done") X(INS_SKIP, "post/insert-skipped")                                                \
    X(IMM0, "imm-rep/0") X(IMM1, "imm-rep/1") X(IMM2, "imm-rep/2+") X(IMM_END, "imm-rep/ends-block")                  \
    X(E_NOSEQ, "block/no-sequences") X(E_TAIL0, "block/tail/0")                                                       \
    X(NS31, "nseq/31") X(NS32, "nseq/32") X(NS33, "nseq/33") X(NS36, "nseq/36") X(NS37, "nseq/37")                    \
    X(NS63, "nseq/63") X(NS64, "nseq/64") X(NS65, "nseq/65") X(NS72, "nseq/72") X(NS73, "nseq/73")                    \
    X(I_NEG, "invariant/negative-read") X(I_PAST, "invariant/read-past-frame")                                        \
    X(I_UNFENCED, "invariant/load-before-fence") X(I_MODEL, "invariant/model-mismatch")                               \
    X(SEQS, "sequences")

enum Cls {
#define X(id, name) C_##id,
    ZDF_CLASSES(X)
#undef X
        C_COUNT
};
const char* const kNames[C_COUNT] = {
#define X(id, name) name,
    ZDF_CLASSES(X)
#undef X
};

struct Seq {
    uint32_t ll, offBase, mlen, offset;
};

struct HostEnv {
    const uint8_t* src;
    uint64_t n;
    std::vector<uint32_t> L, S, Lep, Sep;   // the two tables, and the epoch (fences so far + 1) of each slot's store
    uint32_t epoch = 1;
    uint64_t c[C_COUNT] = {};
    std::vector<Seq> seqs;
    // the block being walked (set by begin_block)
    int bs = 0, be = 0, plow = 0, ilimit = 0, anchor = 0, W = 0;
    uint32_t plowIdx = 0;
    int block_seqs = 0, block_searches = 0, block_found = 0;
    bool saved1 = false, saved2 = false;
    // the walk as seen from the calls
    enum { IDLE, SEARCHED, MATCHED, POST } st = IDLE;
    enum { NONE, REP, LONG, SHORT, LONG1 } pred = NONE, kind = NONE;
    struct Cand { uint32_t v; bool fresh; } lastL{0, false}, lastS{0, false};
    enum { H_OTHER, H_LP, H_SP } h1 = H_OTHER, h2 = H_OTHER;   // the last call (h1) and the one before (h2)
    uint32_t h1v = 0, h2v = 0;
    int rp0 = -1, rp1 = -1;                // positions of the last two r64 calls
    bool r32_seen = false;                 // an r32 since the last short_get: the repcode check of this position
    int r32_pos = 0;
    int ip = 0, ip1 = 0;                   // the searched position and the next one
    uint64_t w0 = 0, w1 = 0;
    int cf_a = 0, cf_b = 0, cf_r = 0;      // the last count_fwd
    bool bwd_seen = false, hl1_put = false, cand_fresh = false;
    int post_puts = 0, imm = 0;

    void hist(int k, uint32_t v) { h2 = h1; h2v = h1v; h1 = (decltype(h1))k; h1v = v; }
    uint64_t rd(int pos, int nb) {
        if (pos < 0) { c[C_I_NEG]++; return 0; }
        if ((uint64_t)pos + nb > n) { c[C_I_PAST]++; return 0; }
        uint64_t v = 0;
        memcpy(&v, src + pos, nb);        // (little-endian host)
        return v;
    }
    // ---- the environment of zdf::dfast_block
    uint32_t r32(int pos) { r32_seen = true; r32_pos = pos; hist(H_OTHER, 0); return (uint32_t)rd(pos, 4); }
    uint64_t r64(int pos) { rp0 = rp1; rp1 = pos; hist(H_OTHER, 0); return rd(pos, 8); }
    uint32_t long_get(uint32_t h) {
        if (Lep[h] == epoch) c[C_I_UNFENCED]++;
        lastL = {L[h], L[h] != 0 && Lep[h] + 1 == epoch};
        hist(H_OTHER, 0);
        return L[h];
    }
    uint32_t short_get(uint32_t h) {
        if (Sep[h] == epoch) c[C_I_UNFENCED]++;
        lastS = {S[h], S[h] != 0 && Sep[h] + 1 == epoch};
        r32_seen = false;
        hist(H_OTHER, 0);
        return S[h];
    }
    void long_put(uint32_t h, uint32_t v) {
        L[h] = v; Lep[h] = epoch;
        if (st == MATCHED) hl1_put = true;
        if (st == POST) post_puts++;
        hist(H_LP, v);
    }
    void short_put(uint32_t h, uint32_t v) {
        S[h] = v; Sep[h] = epoch;
        if (st == POST) post_puts++;
        hist(H_SP, v);
    }
    void fence() {
        if (h2 == H_LP && h1 == H_SP && h1v == h2v && (st == IDLE || st == SEARCHED)) on_search((int)h1v - 2);
        else if (st == POST) close_post();
        else c[C_I_MODEL]++;
        epoch++;
        hist(H_OTHER, 0);
    }
    void reject(bool is_long, const Cand& k, uint64_t want, int nb) {
        if (k.v == 0) c[is_long ? C_RL_EMPTY : C_RS_EMPTY]++;
        else if (k.v <= plowIdx) c[is_long ? C_RL_STALE : C_RS_STALE]++;
        else if (rd((int)k.v - 2, nb) != want) c[is_long ? C_RL_COLL : C_RS_COLL]++;
        else c[C_I_MODEL]++;               // a candidate that matches is no rejection
    }
    bool hits(const Cand& k, uint64_t want, int nb) { return k.v > plowIdx && rd((int)k.v - 2, nb) == want; }
    void on_search(int pos) {
        if (st == SEARCHED && pred != NONE) c[C_I_MODEL]++;   // the walk went on where a match was due
        ip = pos;
        ip1 = rp1;
        if (rp0 != ip || ip1 <= ip) c[C_I_MODEL]++;
        w0 = rd(ip, 8);
        w1 = rd(ip1, 8);
        block_searches++;
        st = SEARCHED;
        if (r32_seen && (uint32_t)rd(r32_pos, 4) == (uint32_t)(w0 >> 8)) { pred = REP; return; }
        if (hits(lastL, w0, 8)) { pred = LONG; return; }
        reject(true, lastL, w0, 8);
        if (hits(lastS, (uint32_t)w0, 4)) { pred = SHORT; return; }
        reject(false, lastS, (uint32_t)w0, 4);
        pred = NONE;
    }
    int count_fwd(int a, int b, int maxn) {
        int r = 0;
        while (r < maxn && rd(a + r, 1) == rd(b + r, 1)) r++;
        c[r == 0 ? C_CF0 : r < 256 ? C_CF1 : r == 256 ? C_CF256 : r < 512 ? C_CF257 : C_CF512]++;
        if (r == maxn) c[C_CF_END]++;
        if (maxn != be - a) c[C_I_MODEL]++;
        cf_a = a; cf_b = b; cf_r = r;
        if (st == SEARCHED) {
            kind = a == ip + 5 ? REP : a == ip + 8 ? LONG : a == ip + 4 ? SHORT : a == ip1 + 8 ? LONG1 : NONE;
            if (kind == NONE || (kind == LONG1 ? SHORT : kind) != pred) c[C_I_MODEL]++;
            if (kind == LONG) cand_fresh = lastL.fresh;          // lastL: idxl0, no long_get since the fence
            if (kind == SHORT) { cand_fresh = lastS.fresh; reject(true, lastL, w1, 8); }   // lastL: idxl1
            if (kind == LONG1) { cand_fresh = lastL.fresh; if (!hits(lastL, w1, 8)) c[C_I_MODEL]++; }
            st = MATCHED;
            bwd_seen = hl1_put = false;
        } else if (st == POST) {
            imm++;
        } else {
            c[C_I_MODEL]++;
        }
        hist(H_OTHER, 0);
        return r;
    }
    int count_bwd(int a, int b, int maxn) {
        int r = 0;
        while (r < maxn && rd(a - 1 - r, 1) == rd(b - 1 - r, 1)) r++;
        if (st != MATCHED || kind == REP || maxn <= 0) c[C_I_MODEL]++;
        c[r == 0 ? C_CU0 : r < 64 ? C_CU1 : r == 64 ? C_CU64 : C_CU65]++;
        if (r == a - anchor) c[C_CU_ANCHOR]++;
        if (r == b - plow) c[C_CU_PLOW]++;
        bwd_seen = true;
        hist(H_OTHER, 0);
        return r;
    }
    void seq(int from, int ll, uint32_t offBase, uint32_t mlen) {
        const int start = from + ll;
        const uint32_t offset = (uint32_t)(cf_a - cf_b);
        if (from != anchor || ll < 0) c[C_I_MODEL]++;
        if (offBase > 3 ? offset + 3 != offBase : offBase != 1) c[C_I_MODEL]++;
        c[ll == 0 ? C_LIT0 : ll < 64 ? C_LIT1 : ll == 64 ? C_LIT64 : ll < 256 ? C_LIT65 : ll == 256 ? C_LIT256 : C_LIT257]++;
        if (ll >= 65536) c[C_LIT_LONG]++;
        if (offset == 1) c[C_OFF1]++;
        else if (offset < 8) c[C_OFF2]++;
        if (offset >= 65536) c[C_OFF64K]++;
        if (offset == (uint32_t)W) c[C_OFF_W]++;
        if (start - (int)offset < bs) c[C_OFF_EARLIER]++;
        if (mlen >= 65539) c[offBase == 1 ? C_ML_LONG_REP : C_ML_LONG]++;
        c[C_SEQS]++;
        block_seqs++;
        seqs.push_back({(uint32_t)ll, offBase, mlen, offset});
        if (st == MATCHED) {
            c[kind == REP ? C_S_REP : kind == LONG ? C_S_LONG : kind == SHORT ? C_S_SHORT : C_S_LONG1]++;
            if (kind == REP) {
                if (ll < 1 || offBase != 1 || hl1_put || bwd_seen) c[C_I_MODEL]++;
            } else {
                const int step = ip1 - ip;
                block_found++;
                if (!bwd_seen) {                        // no room: the match starts at the anchor
                    c[C_CU0]++;
                    if (ll == 0) c[C_CU_ANCHOR]++;
                    else c[C_I_MODEL]++;
                }
                c[step == 1 ? C_STEP1 : step == 2 ? C_STEP2 : step == 3 ? C_STEP3 : C_STEP4]++;
                c[hl1_put ? C_HL1_IN : C_HL1_SKIP]++;
                if (hl1_put != (step < 4)) c[C_I_MODEL]++;
                if (cand_fresh) c[kind == SHORT ? C_FRESH_S : C_FRESH_L]++;
                if (mlen != (uint32_t)cf_r + (kind == SHORT ? 4u : 8u) + (uint32_t)((kind == LONG1 ? ip1 : ip) - start)) c[C_I_MODEL]++;
            }
            st = POST;
            post_puts = imm = 0;
        } else if (st == POST) {                        // an immediate repcode
            if (ll != 0 || offBase != 1 || start != cf_a - 4 || mlen != (uint32_t)cf_r + 4) c[C_I_MODEL]++;
            if (start + (int)mlen > ilimit) c[C_IMM_END]++;
        } else {
            c[C_I_MODEL]++;
        }
        anchor = start + (int)mlen;
        hist(H_OTHER, 0);
    }
    void close_post() {
        c[post_puts ? C_INS_DONE : C_INS_SKIP]++;
        if (!post_puts && (imm || anchor <= ilimit)) c[C_I_MODEL]++;
        if (post_puts && post_puts != 4 + 2 * imm) c[C_I_MODEL]++;
        c[imm == 0 ? C_IMM0 : imm == 1 ? C_IMM1 : C_IMM2]++;
        st = IDLE;
    }
    void begin_block(const zdf::DParams& P, int bs_, int be_, const uint32_t rep[2]) {
        bs = bs_; be = be_;
        W = 1 << P.wlog;
        const int dl = bs > W ? bs - W : 0;
        plow = (be - dl > W) ? be - W : dl;
        plowIdx = (uint32_t)plow + 2;
        ilimit = be - 8;
        anchor = bs;
        block_seqs = block_searches = 0;
        st = IDLE;
        pred = kind = NONE;
        h1 = h2 = H_OTHER;
        const int first = bs == plow;
        c[first ? C_B_FIRST : C_B_LATER]++;
        if (dl > 0) c[C_B_DL]++;
        if (plow > dl) c[C_B_PLOW]++;
        const int ip0 = bs + first;
        const int wlow = (ip0 - dl > W) ? ip0 - W : dl;
        const uint32_t maxRep = (uint32_t)(ip0 - wlow);
        saved2 = rep[1] > maxRep;
        saved1 = rep[0] > maxRep;
        block_found = 0;
        if (saved2) c[C_B_OFF2]++;
        if (saved1) c[C_B_OFF1]++;
        if ((saved1 || saved2) && bs != 0) c[C_B_SAVED_LATER]++;
        if (ip0 + 1 > ilimit) c[C_B_SHORT]++;
    }
    void end_block(int ret_anchor, const uint32_t rep_in[2], const uint32_t rep_out[2]) {
        if (ret_anchor != anchor || anchor > be) c[C_I_MODEL]++;
        if (st == SEARCHED) {
            if (pred != NONE) c[C_I_MODEL]++;
            c[C_S_OUT]++;
        } else if (st == IDLE) {
            if (block_seqs) c[C_S_ENDMATCH]++;
        } else {
            c[C_I_MODEL]++;
        }
        // off2 is 0 until the first stored match of the search (off2 = off1), off1 until the second: a saved offset
        // comes back at the exit where its slot is still 0
        if ((saved2 && block_found == 0) || (saved1 && block_found < 2)) {
            c[C_B_RESTORED]++;
            const uint32_t saved = saved1 ? rep_in[0] : rep_in[1];
            if (rep_out[1] != saved) c[C_I_MODEL]++;
        }
        if (block_seqs == 0) c[C_E_NOSEQ]++;
        if (anchor == be) c[C_E_TAIL0]++;
        switch (block_seqs) {
            case 31: c[C_NS31]++; break; case 32: c[C_NS32]++; break; case 33: c[C_NS33]++; break;
            case 36: c[C_NS36]++; break; case 37: c[C_NS37]++; break; case 63: c[C_NS63]++; break;
            case 64: c[C_NS64]++; break; case 65: c[C_NS65]++; break; case 72: c[C_NS72]++; break;
            case 73: c[C_NS73]++; break; default: break;
        }
    }
};

}  // namespace

extern "C" {

int zdf_census_nclasses(void) { return C_COUNT; }
const char* zdf_census_class_name(int i) { return i >= 0 && i < C_COUNT ? kNames[i] : ""; }

// Walks the frame src[0, n) at level 3.  confirm: one byte per block, 0 where the block's repcodes are not
// confirmed (the reference stored it raw or as RLE; the next block then starts from the repcodes before it), or
// NULL: every searched block confirms.
// seqs: 4 words per stored sequence (literal length, offBase, match length, resolved offset), blocks in order.
// blocks: 4 words per block (sequences, literal bytes with the tail, tail literals, 1 if the block was searched).
// counters: zdf_census_nclasses() words.  Returns the number of blocks, -1: a capacity is too small.
int64_t zdf_census_frame(const uint8_t* src, uint64_t n, const uint8_t* confirm, uint32_t* seqs, uint64_t seq_cap,
                         uint32_t* blocks, uint64_t block_cap, uint64_t* counters) {
    const zdf::DParams P = zdf::params_for(3, n);
    const uint64_t nblocks = n ? (n + P.bsize - 1) / P.bsize : 1;
    if (nblocks > block_cap || n > 0x7fffffffull - 16) return -1;
    HostEnv E;
    E.src = src;
    E.n = n;
    E.L.assign((size_t)1 << P.hlog, 0);
    E.S.assign((size_t)1 << P.clog, 0);
    E.Lep.assign((size_t)1 << P.hlog, 0);
    E.Sep.assign((size_t)1 << P.clog, 0);
    {   // the parameter classes: the clevels row and what ZSTD_adjustCParams_internal changed of it
        const uint8_t rows[4][3] = {{21, 16, 17}, {18, 16, 16}, {17, 15, 16}, {14, 14, 15}};   // W, C, H
        const int tid = n == 0 ? 0 : (n <= 262144) + (n <= 131072) + (n <= 16384);
        E.c[C_ROW0 + tid]++;
        E.c[P.mls == 4 ? C_MLS4 : C_MLS5]++;
        uint32_t srcLog = 6;
        if (n >= 64) { srcLog = 1; while ((1ull << srcLog) < n) srcLog++; }
        const uint32_t w = n && rows[tid][0] > srcLog ? srcLog : rows[tid][0];
        if (w < rows[tid][0]) E.c[C_WLOG_CL]++;
        if (n && rows[tid][2] > w + 1) E.c[C_HLOG_CL]++;
        if (n && rows[tid][1] > w) E.c[C_CLOG_CL]++;
        if (w < 10) E.c[C_WLOG_10]++;
        E.c[nblocks == 1 ? C_BLOCKS1 : nblocks == 2 ? C_BLOCKS2 : C_BLOCKS3]++;
    }
    uint32_t conf[2] = {1u, 4u};                         // repStartValue
    size_t nseq_before = 0;
    for (uint64_t k = 0; k < nblocks; k++) {
        const int bs = (int)(k * P.bsize);
        const int be = (int)(n < (uint64_t)bs + P.bsize ? n : (uint64_t)bs + P.bsize);
        uint32_t* b = blocks + 4 * k;
        if (be - bs < 7) {                               // ZSTD_buildSeqStore: too small, stored raw, nothing searched
            E.c[C_B_RAW]++;
            b[0] = 0; b[1] = (uint32_t)(be - bs); b[2] = (uint32_t)(be - bs); b[3] = 0;
            continue;
        }
        uint32_t rep[2] = {conf[0], conf[1]};
        const uint32_t rep_in[2] = {conf[0], conf[1]};
        E.begin_block(P, bs, be, rep);
        const int anchor = zdf::dfast_block(E, P, bs, be, rep);
        E.end_block(anchor, rep_in, rep);
        uint64_t lits = (uint64_t)(be - anchor);
        for (size_t i = nseq_before; i < E.seqs.size(); i++) lits += E.seqs[i].ll;
        b[0] = (uint32_t)(E.seqs.size() - nseq_before); b[1] = (uint32_t)lits; b[2] = (uint32_t)(be - anchor); b[3] = 1;
        nseq_before = E.seqs.size();
        if (!confirm || confirm[k]) { conf[0] = rep[0]; conf[1] = rep[1]; }
        else E.c[C_B_UNCONF]++;
    }
    if (E.seqs.size() > seq_cap) return -1;
    for (size_t i = 0; i < E.seqs.size(); i++) {
        seqs[4 * i] = E.seqs[i].ll; seqs[4 * i + 1] = E.seqs[i].offBase;
        seqs[4 * i + 2] = E.seqs[i].mlen; seqs[4 * i + 3] = E.seqs[i].offset;
    }
    memcpy(counters, E.c, sizeof(E.c));
    return (int64_t)nblocks;
}

}  // extern "C"

#ifdef ZDF_CENSUS_MAIN
// zstd_dfast_census_walk FILE...: walks each file as one frame, replays its sequences and compares with the file
int main(int argc, char** argv) {
    uint64_t total[C_COUNT] = {};
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<uint8_t> d;
        uint8_t buf[65536];
        for (size_t r; (r = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + r);
        fclose(f);
        const uint64_t n = d.size();
        std::vector<uint8_t> exact(d);                   // (capacity == size: a read past the frame is a heap overflow)
        exact.shrink_to_fit();
        std::vector<uint32_t> seqs(4 * (n / 4 + 16)), blocks(4 * (n / 1024 + 2));
        uint64_t c[C_COUNT];
        const int64_t nb = zdf_census_frame(exact.data(), n, nullptr, seqs.data(), seqs.size() / 4, blocks.data(),
                                            blocks.size() / 4, c);
        if (nb < 0) { fprintf(stderr, "%s: walk failed (%lld)\n", argv[a], (long long)nb); return 1; }
        std::vector<uint8_t> out;
        out.reserve(n);
        const zdf::DParams P = zdf::params_for(3, n);
        size_t s = 0, pos = 0;
        for (int64_t k = 0; k < nb; k++) {
            for (uint32_t i = 0; i < blocks[4 * k]; i++, s++) {
                const uint32_t ll = seqs[4 * s], ml = seqs[4 * s + 2], off = seqs[4 * s + 3];
                out.insert(out.end(), d.begin() + pos, d.begin() + pos + ll);
                pos += ll;
                if (off == 0 || off > out.size()) { fprintf(stderr, "%s: offset %u at %zu\n", argv[a], off, out.size()); return 1; }
                for (uint32_t j = 0; j < ml; j++) out.push_back(out[out.size() - off]);
                pos += ml;
            }
            out.insert(out.end(), d.begin() + pos, d.begin() + pos + blocks[4 * k + 2]);
            pos += blocks[4 * k + 2];
            const size_t end = (size_t)((uint64_t)(k + 1) * P.bsize < n ? (uint64_t)(k + 1) * P.bsize : n);
            if (pos != end) { fprintf(stderr, "%s: block %lld ends at %zu, not %zu\n", argv[a], (long long)k, pos, end); return 1; }
        }
        if (out != d) { fprintf(stderr, "%s: the sequences do not rebuild the input\n", argv[a]); return 1; }
        if (c[C_I_NEG] || c[C_I_PAST] || c[C_I_UNFENCED] || c[C_I_MODEL]) {
            fprintf(stderr, "%s: invariant counters %llu %llu %llu %llu\n", argv[a], (unsigned long long)c[C_I_NEG],
                    (unsigned long long)c[C_I_PAST], (unsigned long long)c[C_I_UNFENCED], (unsigned long long)c[C_I_MODEL]);
            return 1;
        }
        for (int i = 0; i < C_COUNT; i++) total[i] += c[i];
        printf("%s: %llu bytes, %lld blocks, %llu sequences\n", argv[a], (unsigned long long)n, (long long)nb,
               (unsigned long long)c[C_SEQS]);
    }
    int reached = 0;
    for (int i = 0; i < C_COUNT; i++) reached += total[i] != 0;
    printf("%d files, %d of %d classes reached\n", argc - 1, reached, (int)C_COUNT);
    return 0;
}
#endif
