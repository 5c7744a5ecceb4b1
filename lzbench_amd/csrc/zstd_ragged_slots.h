// lzbench_amd/csrc/zstd_ragged_slots.h -- slot arithmetic of the compact layout of ragged zstd compression
// (include/lzbench_hip.h 3c, zstd_ragged_compact_hip.hip): every chunk's staging slot and scratch slot are sized
// from the chunk's own size and level and placed by an exclusive scan, so temp grows with the batch's total
// bytes, not nchunks x (the slots of the largest chunk).  One copy of the arithmetic for the slot-size kernel,
// the sizing function and the host mirror of the placement: the sizes here are what the two kernel bodies
// (zstdc_match_body.inc, zstdc_entropy_body.inc) address for a frame of n bytes alone.
// Include after zstdc.h: the sizes come from its params_for and layout_for (host + device).  api.cpp, which
// does not compile that header, reaches the functions through the host wrappers of zstd_ragged_compact_hip.hip
// (launch.h).
#pragma once
#include "launch.h"
#include "ragged_slots.h"

// staging slot of a chunk of n bytes: ZSTD_COMPRESSBOUND(n) + 16 bytes, 256-aligned
// = lzh_stage_stride(LZH_CODEC_ZSTD, n)
LZH_HD uint64_t lzh_zslot_stage_bytes(uint64_t n) {
    const uint64_t bound = n + (n >> 8) + (n < (128u << 10) ? ((128u << 10) - n) >> 11 : 0);
    return lzh_slot_align(bound + 16);
}

// The parameters that lay a chunk's scratch slot out.  Size 0 is ZSTD_getParams' "unknown size", a full 128 KiB
// block; an empty frame touches only the first 1024 bytes of its scratch (the match body returns after the
// header words, the entropy body after the frame's 9 bytes), so its slot is that of a 1-byte chunk, the
// convention of the uniform-slot calls (api.cpp zstd_ragged_temp, lzh_launch_zstd_ragged).
LZH_HD zc::ZParams lzh_zslot_params(int level, uint64_t n) { return zc::params_for(level, n ? n : 1); }

// scratch slot of a chunk of n bytes at `level`: header and Huffman table, sequences, literals, block attempt,
// one Huffman stream (each for the chunk's own block size) and the chunk's own hash table of 4 << hashLog bytes
// at tab_off (the global table and the save between blocks; always included: which table kind a launch uses
// depends on the batch's max_bytes).  0 where the level has no fast-strategy row for n.
LZH_HD zc::Layout lzh_zslot_layout(const zc::ZParams& P) { return zc::layout_for(P.bsize, P.hlog); }
LZH_HD uint64_t lzh_zslot_scratch_bytes(int level, uint64_t n) {
    const zc::ZParams P = lzh_zslot_params(level, n);
    return P.ok ? lzh_zslot_layout(P).stride : 0;
}

// The largest hashLog of any size up to max_bytes.  hashLog is not monotone in n: it drops where n enters the next
// row of clevels.h (level 1: 15 at 16384 bytes, 13 at 16385).  Inside a row hashLog = min(row, windowLog + 1) does
// not shrink and the rows end at powers of two, so the largest one up to max_bytes is that of max_bytes itself or
// of a power of two below it (lzh_zstd_scratch_stride's loop).  Non-decreasing in max_bytes.
LZH_HD uint32_t lzh_zslot_hlog_worst(int level, uint64_t max_bytes) {
    const uint64_t geo = max_bytes ? max_bytes : 1;
    uint32_t hmax = zc::params_for(level, geo).hlog;
    for (int lg = 0; lg <= 24 && (1ull << lg) < geo; lg++) {
        const zc::ZParams Q = zc::params_for(level, 1ull << lg);
        if (Q.ok && Q.hlog > hmax) hmax = Q.hlog;
    }
    return hmax;
}

// The largest scratch slot of any size up to max_bytes (the slot is not monotone in n either): the block size,
// min(n, 128 KiB), never shrinks, so the block size of max_bytes with the largest hashLog bounds every slot.
// = lzh_zstd_scratch_stride(max_bytes, level)
LZH_HD uint64_t lzh_zslot_scratch_worst(int level, uint64_t max_bytes) {
    const zc::ZParams P = zc::params_for(level, max_bytes ? max_bytes : 1);
    return P.ok ? zc::layout_for(P.bsize, lzh_zslot_hlog_worst(level, max_bytes)).stride : 0;
}

// The two regions that hold the slots of every batch of at most nchunks chunks, each of at most max_bytes, that
// sums to at most total bytes.
// Staging: ZSTD_COMPRESSBOUND(n) <= n + n / 256 + 64, + 16, + at most 255 of alignment: the sum over a batch is at
// most total + total / 256 + nchunks x 335.
// Scratch, the areas before the table, for a block size b = min(n, 128 KiB): 1024 + (2 b + 128 + 255)
// + (b + 64 + 255) + (4 b + 4096 + 255) + (b + 256 + 255) <= 8 b + 6588.  The sum of b over a batch is at most total
// and at most nchunks x min(max_bytes, 128 KiB): one large chunk pays for one block, not for its size.
// Scratch, the table: 4 << hashLog bytes with hashLog <= windowLog + 1 and windowLog <= max(6, ceil(log2 n)):
// 2^windowLog < 2 n from 64 bytes on, so the table is under 16 n there and 512 bytes below 64 bytes -- several
// times a small chunk, which is why a byte of a batch of small chunks costs 24 bytes of scratch and not 8.  It is
// also at most 4 << (the largest hashLog up to max_bytes), 32 KiB at the negative levels.  The sum over a batch is
// at most 16 x total + nchunks x 512 and at most nchunks x that largest table.
// An empty chunk takes the slot of one byte (8 more than the formulas give for n = 0): 6588 + 8 <= 6656 a chunk.
// The sum of the slots is also at most nchunks x the worst slot of any size up to max_bytes (the staging slot is
// non-decreasing in n; lzh_zslot_scratch_worst above), which keeps the answer within the uniform-slot layout's.
// Every term is non-decreasing in each argument, so both answers are.
// Range: as lzh_compact_regions, u64 arithmetic without overflow checks (16 x total needs total < 2^60).
LZH_HD uint64_t lzh_zslot_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
LZH_HD LzhCompactRegions lzh_zslot_regions(int level, uint64_t total, uint64_t max_bytes, uint64_t nchunks) {
    const uint64_t bmax = lzh_zslot_min(max_bytes ? max_bytes : 1, 131072);
    const uint64_t tmax = 4ull << lzh_zslot_hlog_worst(level, max_bytes);
    const uint64_t st = total + (total >> 8) + nchunks * 335;
    const uint64_t sc = lzh_zslot_min(8 * total, nchunks * 8 * bmax) + nchunks * 6656 +
                        lzh_zslot_min(16 * total + nchunks * 512, nchunks * tmax);
    LzhCompactRegions r;   // (recs: the scratch region)
    r.stage = lzh_slot_align(lzh_zslot_min(st, nchunks * lzh_zslot_stage_bytes(max_bytes)));
    r.recs = lzh_slot_align(lzh_zslot_min(sc, nchunks * lzh_zslot_scratch_worst(level, max_bytes)));
    return r;
}
