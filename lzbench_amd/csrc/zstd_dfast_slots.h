// lzbench_amd/csrc/zstd_dfast_slots.h -- slot arithmetic of ragged zstd level-3 batches (include/lzbench_hip.h 3e,
// zstd_dfast_ragged_hip.hip): the sibling of zstd_ragged_slots.h for the double-fast strategy, whose frames keep two
// tables (long: 4 << hashLog bytes, short: 4 << chainLog) after the fast levels' areas.  One copy of the arithmetic
// for the slot-size kernel, the compact kernels' area offsets, the sizing functions and the host mirror of the
// placement (api.cpp).
// Plain C++ on the host: the level-3 parameters come from zstd_dfast_parse.h, and the areas before the tables are
// restated here (lzh_zdslot_layout) so that nothing of zstdc.h is needed; lzh_launch_zstd_dfast_ragged
// refuses to launch where this copy and that header's layout_for disagree.
#pragma once
#include "ragged_slots.h"
#include "zstd_dfast_parse.h"

// staging slot of a chunk of n bytes: ZSTD_COMPRESSBOUND(n) + 16 bytes, 256-aligned
// = lzh_stage_stride(LZH_CODEC_ZSTD, n) = lzh_zslot_stage_bytes(n) of zstd_ragged_slots.h (the frames have that
// codec's bound: the entropy stage is the same)
LZH_HD uint64_t lzh_zdslot_stage_bytes(uint64_t n) {
    const uint64_t bound = n + (n >> 8) + (n < (128u << 10) ? ((128u << 10) - n) >> 11 : 0);
    return lzh_slot_align(bound + 16);
}

// The parameters that lay a chunk's scratch slot out.  Size 0 is ZSTD_getParams' "unknown size", a full 128 KiB
// block; an empty frame touches only the first 1024 bytes of its scratch (the match body returns after the header
// words, the entropy body after the frame's 9 bytes), so its slot is that of a 1-byte chunk: the convention of 3c.
LZH_HD zdf::DParams lzh_zdslot_params(uint64_t n) { return zdf::params_for(3, n ? n : 1); }

// A chunk's scratch slot: the areas of zc::layout_for (zstdc.h) for the chunk's own block size -- 1024 bytes of
// header and Huffman table, sequences, literals, the block attempt, one Huffman stream, each 256-aligned -- then at
// tab_off the long table and right after it the short one, each of the chunk's own level-3 row.  stride: the slot.
struct LzhZdLayout {
    uint64_t seq_off, lit_off, att_off, tmp_off, tab_off, stride;
};
LZH_HD uint64_t lzh_zdslot_areas(uint64_t bsize, LzhZdLayout& L) {
    L.seq_off = 1024;
    L.lit_off = L.seq_off + lzh_slot_align((bsize / 4 + 16) * 8);
    L.att_off = L.lit_off + lzh_slot_align(bsize + 64);
    L.tmp_off = L.att_off + lzh_slot_align(bsize * 4 + 4096);
    L.tab_off = L.tmp_off + lzh_slot_align(bsize + 256);
    return L.tab_off;
}
LZH_HD LzhZdLayout lzh_zdslot_layout(const zdf::DParams& P) {
    LzhZdLayout L;
    L.stride = lzh_slot_align(lzh_zdslot_areas(P.bsize, L) + (4ull << P.hlog) + (4ull << P.clog));
    return L;
}
LZH_HD uint64_t lzh_zdslot_scratch_bytes(uint64_t n) { return lzh_zdslot_layout(lzh_zdslot_params(n)).stride; }

// The largest hashLog and chainLog of any size up to max_bytes, without relying on either being monotone in n (at
// level 3 they are: the rows {W, C, H} of clevels.h grow with the size class, {14,14,15}, {17,15,16}, {18,16,16},
// {21,16,17}; at the fast levels hashLog drops between rows, zstd_ragged_slots.h).  Inside a row
// hashLog = min(row, windowLog + 1) and chainLog = min(row, windowLog) do not shrink as n grows and the rows end at
// powers of two, so the largest of each up to max_bytes is that of max_bytes itself or of a power of two below it;
// sizes under 64 bytes share the parameters of 1 byte (lzh_zstd_dfast_scratch_stride's loop).
// Both are non-decreasing in max_bytes: the largest over a growing set.
LZH_HD void lzh_zdslot_logs_worst(uint64_t max_bytes, uint32_t& hmax, uint32_t& cmax) {
    const uint64_t geo = max_bytes ? max_bytes : 1;
    const zdf::DParams P = zdf::params_for(3, geo), T = zdf::params_for(3, 1);
    hmax = P.hlog > T.hlog ? P.hlog : T.hlog;
    cmax = P.clog > T.clog ? P.clog : T.clog;
    for (int lg = 6; lg <= 24 && (1ull << lg) < geo; lg++) {
        const zdf::DParams Q = zdf::params_for(3, 1ull << lg);
        if (Q.hlog > hmax) hmax = Q.hlog;
        if (Q.clog > cmax) cmax = Q.clog;
    }
}
LZH_HD uint64_t lzh_zdslot_tables_worst(uint64_t max_bytes) {
    uint32_t h, c;
    lzh_zdslot_logs_worst(max_bytes, h, c);
    return (4ull << h) + (4ull << c);
}

// The largest scratch slot of any size up to max_bytes: the block size, min(n, 128 KiB), never shrinks, so the areas
// of max_bytes' block size with the largest of each table bound every slot.
// = lzh_zstd_dfast_scratch_stride(max_bytes) for max_bytes >= 1 (zstdc_dfast_hip.hip), the uniform-slot stride.
LZH_HD uint64_t lzh_zdslot_scratch_worst(uint64_t max_bytes) {
    LzhZdLayout L;
    return lzh_slot_align(lzh_zdslot_areas(lzh_zdslot_params(max_bytes).bsize, L) + lzh_zdslot_tables_worst(max_bytes));
}

// The two regions that hold the slots of every batch of at most nchunks chunks, each of at most max_bytes, that
// sums to at most total bytes.
// Staging (as zstd_ragged_slots.h): ZSTD_COMPRESSBOUND(n) <= n + n / 256 + 64, + 16, + at most 255 of alignment:
// the sum over a batch is at most total + total / 256 + nchunks x 335.
// Scratch, the areas before the tables, for a block size b: 1024 + (2 b + 128 + 255) + (b + 64 + 255)
// + (4 b + 4096 + 255) + (b + 256 + 255) <= 8 b + 6588.  b = min(2^windowLog, 128 KiB, n) is min(n, 128 KiB): the
// row's window is at least the row's largest size (2^14, 2^17, 2^18; 2^21 above) and the adjusted one,
// 2^ceil(log2 n), at least n.  So the sum of b over a batch is at most total and at most
// nchunks x min(max_bytes, 128 KiB): one large chunk pays for one block, not for its size.
// Scratch, the tables.  From 64 bytes on ZSTD_adjustCParams_internal leaves windowLog <= ceil(log2 n), so
// 2^windowLog < 2 n; hashLog <= windowLog + 1 and chainLog <= windowLog, so the long table, 4 << hashLog, is at most
// 8 x 2^windowLog < 16 n and the short one, 4 << chainLog, at most 4 x 2^windowLog < 8 n: under 24 n together.  Below
// 64 bytes the adjusted windowLog is 6 (ZSTD_HASHLOG_MIN; the floor of 10 is applied to the window after the tables
// are derived), hashLog 7 and chainLog 6: 512 + 256 = 768 bytes, which 24 n does not cover for n < 32.  So a chunk's
// tables are at most 24 n + 768, the sum over a batch at most 24 x total + nchunks x 768 -- a byte of a batch of small
// chunks costs 32 bytes of scratch -- and also at most nchunks x (the largest long table + the largest short table
// up to max_bytes).  Both tables are multiples of 256, so the slot's own alignment adds nothing to the 6588.
// An empty chunk takes the slot of one byte (8 more than the formulas give for n = 0): 6588 + 8 <= 6656 a chunk,
// the term of zstd_ragged_slots.h.
// The sum of the slots is also at most nchunks x the worst slot of any size up to max_bytes (lzh_zdslot_scratch_worst;
// the staging slot is non-decreasing in n), which keeps the answer within the uniform-slot layout's.
// Every term is non-decreasing in each argument, so both answers are.
// Range: as lzh_compact_regions, u64 arithmetic without overflow checks (24 x total needs total < 2^59).
LZH_HD uint64_t lzh_zdslot_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
LZH_HD LzhCompactRegions lzh_zdslot_regions(uint64_t total, uint64_t max_bytes, uint64_t nchunks) {
    const uint64_t bmax = lzh_zdslot_min(max_bytes ? max_bytes : 1, 131072);
    const uint64_t st = total + (total >> 8) + nchunks * 335;
    const uint64_t sc = lzh_zdslot_min(8 * total, nchunks * 8 * bmax) + nchunks * 6656 +
                        lzh_zdslot_min(24 * total + nchunks * 768, nchunks * lzh_zdslot_tables_worst(max_bytes));
    LzhCompactRegions r;   // (recs: the scratch region)
    r.stage = lzh_slot_align(lzh_zdslot_min(st, nchunks * lzh_zdslot_stage_bytes(max_bytes)));
    r.recs = lzh_slot_align(lzh_zdslot_min(sc, nchunks * lzh_zdslot_scratch_worst(max_bytes)));
    return r;
}
