// lzbench_amd/csrc/zstd_split_slots.h -- area arithmetic of the compact layout of the ragged zstd split decoder
// (include/lzbench_hip.h 3g, zstd_ragged_split_compact_hip.hip, and the debug calls of 3c): every frame's temp area is laid out
// for the frame's own decoded size and placed by an exclusive scan, and the Huffman job list holds the sum of the
// frames' own block slots, so temp grows with the batch's total bytes, not nchunks x (the area of the largest
// chunk).  One copy of the arithmetic, host and device: the sizes here are what the four kernel bodies address for
// a frame of n bytes alone.
// Include after decode_hip.hip: everything comes from its zsplit::zlayout (host + device).  api.cpp, which cannot
// include that file, reaches the functions through the host wrappers of zstd_ragged_split_hip.hip (launch.h).
#pragma once
#include "launch.h"
#include "ragged_slots.h"

// the area of a frame of n bytes: zlayout(n).stride, a multiple of 256 -- bmax = ceil(n / 128 KiB) + 1 block slots
// (a block's fields, its output position, its sequence tables and its Huffman table) and smax = n / 4 + 64
// sequence records of 8 bytes
LZH_HD uint64_t lzh_zsplit_area_bytes(uint64_t n) { return zsplit::zlayout(n).stride; }
// the Huffman jobs a frame of n bytes can post: one per block slot
LZH_HD uint64_t lzh_zsplit_jobs(uint64_t n) { return zsplit::zlayout(n).bmax; }
// a block slot's bytes (the layout of one block and no records, up to the records)
LZH_HD uint64_t lzh_zsplit_block_bytes() { return zsplit::ZLayout{1, 0, 0}.seqs(); }

// The two regions that hold the areas and the jobs of every batch of at most nchunks frames, each of at most
// max_bytes, that sums to at most total bytes.
// Jobs: bmax(n) = ceil(n / 128 KiB) + 1.  Over a batch the ceilings sum to at most total / 128 KiB (the whole
// blocks) + nchunks (a started block a frame), so the jobs to at most total / 131072 + 2 x nchunks.
// Areas: area(n) = bmax(n) x B + 8 x (n / 4 + 64), rounded up to 256, with B = lzh_zsplit_block_bytes() (8,760).
// The records are at most 2 n + 512 bytes and the rounding at most 255, so the sum over a batch is at most
// 2 x total + B x (total / 131072 + 2 x nchunks) + nchunks x 767: twice the batch, a block slot per 128 KiB of it,
// and 2 B + 767 = 18,287 bytes a frame.
// Both are also at most nchunks x the value for max_bytes (bmax and the area are non-decreasing in n), which keeps
// the answers within the uniform-slot layout's: the smaller of the two.  Every term is non-decreasing in each
// argument, so both answers are.
// Range: as lzh_zslot_regions, u64 arithmetic without overflow checks (2 x total needs total < 2^63).
// (LzhZsplitRegions, launch.h: {area bytes, Huffman jobs})
LZH_HD LzhZsplitRegions lzh_zsplit_regions(uint64_t total, uint64_t max_bytes, uint64_t nchunks) {
    const uint64_t B = lzh_zsplit_block_bytes();
    const uint64_t jb = (total >> 17) + 2 * nchunks;
    const uint64_t ju = nchunks * lzh_zsplit_jobs(max_bytes);
    const uint64_t ab = 2 * total + B * jb + nchunks * (64 * 8 + 255);
    const uint64_t au = nchunks * lzh_zsplit_area_bytes(max_bytes);
    LzhZsplitRegions r;
    r.areas = lzh_slot_align(ab < au ? ab : au);
    r.jobs = jb < ju ? jb : ju;
    return r;
}
