// lzbench_amd/csrc/ragged_slots.h -- slot arithmetic of the compact ragged compress layout (include/lzbench_hip.h
// 3b, ragged_compact_hip.hip): every chunk's staging slot and record slot are sized from the chunk's own size
// and placed by an exclusive scan, so temp grows with the batch's total bytes, not nchunks x the largest chunk.
// One copy of the arithmetic for the slot-size kernel, the sizing function and the host mirror of the placement
// (api.cpp): the sizes here are what the kernel bodies (*_body.inc) address for a chunk of n bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LZH_HD __host__ __device__ __forceinline__

constexpr int kLzhSlotLz4 = 0, kLzhSlotSnappy = 1;          // = LZH_CODEC_LZ4, LZH_CODEC_SNAPPY
constexpr uint64_t kLzhSnFragRecBytes = (16384 + 32) * 8;   // = kFragRecs * 8 (snappyc.h), a multiple of 256

LZH_HD uint64_t lzh_slot_align(uint64_t v) { return (v + 255) & ~(uint64_t)255; }

// staging slot of a chunk of n bytes: the codec's bound (LZ4_compressBound, snappy's MaxCompressedLength) + 16
// bytes of slack for the emit kernels' dword stores = lzh_stage_stride(codec, n)
LZH_HD uint64_t lzh_slot_stage_bytes(int codec, uint64_t n) {
    const uint64_t bound = codec == kLzhSlotLz4 ? n + n / 255 + 16 : 32 + n + n / 6;
    return lzh_slot_align(bound + 16);
}

// record slot of a chunk of n bytes (8 bytes per sequence; a sequence covers at least 4 input bytes).
// LZ4: lzh_lz4_rec_stride(n).  snappy in a batch whose chunks have one fragment (max_bytes <= 64 KiB):
// lzh_snappy_rec_stride(n).  snappy in a batch with more fragments per chunk (multi): fragment f's records start
// at record f * kFragRecs of the slot whatever the chunk's own size, so a chunk of nf fragments has nf - 1 whole
// fragment strides and the records of its last fragment (n / 4 copies and the closing literal record, as the
// single-fragment layout sizes them); an empty chunk has no records.
LZH_HD uint64_t lzh_slot_rec_bytes(int codec, uint64_t n, bool multi) {
    if (codec == kLzhSlotLz4) return lzh_slot_align((n / 4 + 4) * 8);
    if (!multi) return lzh_slot_align((n / 4 + 8) * 8);
    if (n == 0) return 0;
    const uint64_t nf = (n + 65535) >> 16, last = n - ((nf - 1) << 16);
    return (nf - 1) * kLzhSnFragRecBytes + lzh_slot_align((last / 4 + 8) * 8);
}

// The two regions that hold the slots of every batch of at most nchunks chunks, each of at most max_bytes, that
// sums to at most total bytes.  Both slot functions are at most a x n + c (floors of n / 255, n / 6, n / 4 add up
// to at most the floor of the total; the 256-alignment costs at most 255 per chunk; the multi-fragment snappy
// layout adds 256 bytes per whole fragment, at most n / 256), so the sum over a batch is at most
// a x total + nchunks x c.  It is also at most nchunks x the slot of max_bytes (both functions are
// non-decreasing in n): the smaller of the two.  Both answers are non-decreasing in each argument.
// Range: u64 arithmetic without overflow checks.  A launchable batch has nchunks < 2^31 and max_bytes <= 16 MiB
// (slots under 2^26 bytes), so the products stay under 2^57 and 2.2 x total needs total < 2^62; the sizing
// function takes any size_t, and past those values its answer wraps and the monotonicity no longer holds.
struct LzhCompactRegions { uint64_t stage, recs; };
LZH_HD LzhCompactRegions lzh_compact_regions(int codec, uint64_t total, uint64_t max_bytes, uint64_t nchunks) {
    const bool multi = max_bytes > 65536;
    uint64_t st, rc;
    if (codec == kLzhSlotLz4) {
        st = total + total / 255 + nchunks * (32 + 255);
        rc = 2 * total + nchunks * (32 + 255);
    } else {
        st = total + total / 6 + nchunks * (48 + 255);
        rc = 2 * total + (multi ? total / 256 : 0) + nchunks * (64 + 255);
    }
    const uint64_t st_u = nchunks * lzh_slot_stage_bytes(codec, max_bytes);
    const uint64_t rc_u = nchunks * lzh_slot_rec_bytes(codec, max_bytes, multi);
    LzhCompactRegions r;
    r.stage = lzh_slot_align(st < st_u ? st : st_u);
    r.recs = lzh_slot_align(rc < rc_u ? rc : rc_u);
    return r;
}

// ---- device side, for the two compact translation units (ragged_compact_hip.hip, zstd_ragged_compact_hip.hip;
// after common.h, whose LZH_WAVE is the guard: api.cpp includes this file for the arithmetic above alone) ----
#ifdef LZH_WAVE
#include "launch.h"

// A chunk's slot, for the bodies' `stride`: chunk * slot is its scanned offset, a conversion to an integer its size
struct CompactSlot {
    uint64_t off;     // from the region's base (a multiple of 256)
    uint32_t bytes;
    // (explicit: only the bodies' casts `(uint32_t)stride` / `(uint64_t)stride` read the size; any other arithmetic
    // on a slot, or passing one where an integer is expected, does not compile)
    __device__ __forceinline__ explicit operator uint32_t() const { return bytes; }
    __device__ __forceinline__ explicit operator uint64_t() const { return bytes; }
};
__device__ __forceinline__ uint64_t operator*(uint64_t, CompactSlot s) { return s.off; }
// The zstd bodies (zstd_ragged_compact_hip.hip, zstd_dfast_ragged_hip.hip) pass a slot where they mean its size,
// `out.init(stage + f * stride, stride)`: the conversion that the LZ4 / snappy bodies must spell as a cast is
// implicit for them
struct ZstdSlot : CompactSlot {
    __device__ __forceinline__ operator uint64_t() const { return bytes; }
};

// Chunk i of a compact batch: ragged_span's pointer and size and the chunk's two slots, loaded once and
// wave-uniform.  false = not processed (over max_bytes, or a slot that ends past its region).
__device__ __forceinline__ bool compact_span(const void* const* ptrs, const uint64_t* bytes, uint64_t i,
                                             uint64_t max_bytes, const LzhCompactLayout& L, const uint8_t*& p, int& n,
                                             CompactSlot& stage_slot, CompactSlot& rec_slot) {
    if (!ragged_span(ptrs, bytes, i, max_bytes, p, n)) return false;
    stage_slot.off = uni64(L.stage_off[i]);
    stage_slot.bytes = uni(L.stage_sz[i]);
    rec_slot.off = uni64(L.rec_off[i]);
    rec_slot.bytes = uni(L.rec_sz[i]);
    return stage_slot.off + stage_slot.bytes <= L.stage_cap && rec_slot.off + rec_slot.bytes <= L.rec_cap;
}
#endif
