// lzbench_amd/csrc/zstd_dfast_ragged_hip.hip -- zstd level 3 (the double-fast strategy) on ragged batches
// (include/lzbench_hip.h 3e): the chunks of a batch are given by device arrays of pointers and sizes, chunk i becomes
// the frame lzh_compress_async(LZH_CODEC_ZSTD_DFAST, 3, ..) writes for a chunk of that size alone.
//
// The kernel bodies are the uniform level-3 kernels' text (zstdc_dfast_match_body.inc; zstdc_entropy_body.inc with
// LZH_ZSTD_STRATEGY 2 and zdf::entropy_params), unchanged, behind another frame lookup, as zstd_ragged_hip.hip and
// zstd_ragged_compact_hip.hip do it for the fast levels:
//
//   lzh_zstd_dfast_match_ragged_kernel / lzh_zstd_dfast_entropy_ragged_kernel     uniform slots: ragged_span
//       (common.h); frame i's staging slot and scratch area are slot i of the batch's, each sized for max_bytes
//       (lzh_zstd_dfast_scratch_stride) and reached through descriptors of that size or less;
//   lzh_zstd_dfast_compact_slots_kernel                     chunk i's two slot sizes (zstd_dfast_slots.h)
//   lzh_zstd_dfast_match_compact_kernel / lzh_zstd_dfast_entropy_compact_kernel   compact layout: compact_span
//       (ragged_slots.h) through ZstdSlot; the five area offsets are locals laid out for the chunk's own parameters
//       (lzh_zdslot_layout: the layout whose stride is the slot's size), so every buffer descriptor the bodies build
//       is bounded by the chunk's own slot.
//
// A frame's parameters -- window, block size, the two tables' sizes -- come from the frame's own size on the device
// (zdf::params_for(3, nf)); max_bytes sizes the uniform slots and bounds the number of block launches, never bytes.
// The long and the short table of a frame (4 << hashLog and 4 << chainLog bytes of its own row) sit at tab_off of
// its scratch, are zeroed at block 0 and kept across the frame's blocks, as in the uniform kernel.  An empty chunk
// takes the slot of a 1-byte chunk and becomes the 9-byte frame.  A chunk whose device-side size passes max_bytes,
// or (compact) one with a slot that ends past its region, is not processed: the entropy kernel of block 0 writes
// csizes[i] = 0 and no kernel touches a slot for it.
// Scan and pack are the existing ones (lzh_launch_compact_scans, lzh_launch_pack_ragged / lzh_launch_pack_compact).
// The device functions are those of zstdc_dfast.h (and through it of zstdc.h), compiled with the flags of
// zstdc_dfast_hip.hip; nothing here changes the uniform kernels' code.
#include "zstdc_dfast.h"
#include "zstd_dfast_slots.h"

// ---------------------------------------------------------------------------------- uniform slots
// one wave per chunk; block k of every chunk (a chunk of fewer blocks returns at once)
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_dfast_match_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level,
                                   int k, uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off,
                                   uint64_t tab_off) {
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint64_t ioff = 0;
    const uint8_t* in;
    int sn;
    if (!ragged_span(in_ptrs, in_bytes, f, max_bytes, in, sn)) return;
    const uint64_t nf = (uint64_t)sn;
    const uint64_t in_readable = nf + 16;
#include "zstdc_dfast_match_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_dfast_entropy_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level,
                                     int k, uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off,
                                     uint64_t att_off, uint64_t tmp_off, uint8_t* stage, uint64_t stride,
                                     uint32_t* csizes) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(sizeof(ze::Lds) + 3) / 4];
    LDSA ze::Lds& L = *(LDSA ze::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint64_t ioff = 0;
    const uint8_t* in;
    int sn;
    if (!ragged_span(in_ptrs, in_bytes, f, max_bytes, in, sn)) {
        if (lane == 0 && k == 0) csizes[f] = 0;
        return;
    }
    const uint64_t nf = (uint64_t)sn;
    const uint64_t in_readable = nf + 16;
    // (the body asks params_for(level, nf) for the frame's parameters: here that name is the level-3 row)
    const auto params_for = [](int lv, uint64_t n) { return zdf::entropy_params(lv, n); };
#include "zstdc_entropy_body.inc"
}

// ---------------------------------------------------------------------------------- compact layout
extern "C" __global__ void __launch_bounds__(256)
lzh_zstd_dfast_compact_slots_kernel(const uint64_t* in_bytes, uint64_t max_bytes, uint32_t* stage_sz,
                                    uint32_t* scratch_sz, uint32_t nchunks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchunks) return;
    const uint64_t b = in_bytes[i];
    const bool over = b > max_bytes;
    stage_sz[i] = over ? 0u : (uint32_t)lzh_zdslot_stage_bytes(b);
    scratch_sz[i] = over ? 0u : (uint32_t)lzh_zdslot_scratch_bytes(b);
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_dfast_match_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level,
                                    int k, uint8_t* scratch, const LzhCompactLayout C) {
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint64_t ioff = 0;
    const uint8_t* in;
    int sn;
    ZstdSlot stride, fstride;
    if (!compact_span(in_ptrs, in_bytes, f, max_bytes, C, in, sn, stride, fstride)) return;
    const uint64_t nf = (uint64_t)sn;
    const uint64_t in_readable = nf + 16;
    const LzhZdLayout Lo = lzh_zdslot_layout(lzh_zdslot_params(nf));
    const uint64_t seq_off = Lo.seq_off, lit_off = Lo.lit_off, tab_off = Lo.tab_off;
#include "zstdc_dfast_match_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_dfast_entropy_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level,
                                      int k, uint8_t* scratch, uint8_t* stage, uint32_t* csizes,
                                      const LzhCompactLayout C) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(sizeof(ze::Lds) + 3) / 4];
    LDSA ze::Lds& L = *(LDSA ze::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint64_t ioff = 0;
    const uint8_t* in;
    int sn;
    ZstdSlot stride, fstride;
    if (!compact_span(in_ptrs, in_bytes, f, max_bytes, C, in, sn, stride, fstride)) {
        if (lane == 0 && k == 0) csizes[f] = 0;
        return;
    }
    const uint64_t nf = (uint64_t)sn;
    const uint64_t in_readable = nf + 16;
    const LzhZdLayout Lo = lzh_zdslot_layout(lzh_zdslot_params(nf));
    const uint64_t seq_off = Lo.seq_off, lit_off = Lo.lit_off, att_off = Lo.att_off, tmp_off = Lo.tmp_off;
    const auto params_for = [](int lv, uint64_t n) { return zdf::entropy_params(lv, n); };
#include "zstdc_entropy_body.inc"
}

// ------------------------------------------------------------------------- host side: arithmetic, launchers
#include <algorithm>

LzhCompactRegions lzh_zstd_dfast_compact_regions(uint64_t total, uint64_t max_bytes, uint64_t nchunks) {
    return lzh_zdslot_regions(total, max_bytes, nchunks);
}

LzhCompactRegions lzh_zstd_dfast_compact_slot(uint64_t n) {
    return {lzh_zdslot_stage_bytes(n), lzh_zdslot_scratch_bytes(n)};
}

// The geometry of a launch: the block size of max_bytes (a batch of empty chunks: that of 1-byte chunks, as api.cpp
// sizes the slots), the block launches ceil(max(max_bytes, 1) / bsize), and the check that the slot arithmetic's
// restated areas (zstd_dfast_slots.h) are those of the kernels' layout_for.
static bool dfast_ragged_geo(uint64_t max_bytes, int level, Layout& Lo, uint32_t& nblocks) {
    const uint64_t geo = std::max<uint64_t>(max_bytes, 1);
    const zdf::DParams PF = zdf::params_for(level, geo);
    if (!PF.ok) return false;
    Lo = layout_for(PF.bsize, 16);   // offsets below tab_off do not depend on hlog
    LzhZdLayout own;
    if (lzh_zdslot_areas(PF.bsize, own) != Lo.tab_off || own.seq_off != Lo.seq_off || own.lit_off != Lo.lit_off ||
        own.att_off != Lo.att_off || own.tmp_off != Lo.tmp_off)
        return false;
    nblocks = (uint32_t)((geo + PF.bsize - 1) / PF.bsize);
    return true;
}

hipError_t lzh_launch_zstd_dfast_ragged(const LzhBatch& B, int level, const LzhSlots& S, uint32_t* csizes,
                                        hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    Layout Lo;
    uint32_t nblocks;
    if (!dfast_ragged_geo(B.max_bytes, level, Lo, nblocks)) return hipErrorInvalidValue;
    if (S.rec_stride < lzh_zdslot_scratch_worst(B.max_bytes)) return hipErrorInvalidValue;
    // (every launch on s: a captured call has no parallel branches)
    for (uint32_t k = 0; k < std::max(nblocks, 1u); k++) {
        hipLaunchKernelGGL(lzh_zstd_dfast_match_ragged_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes,
                           B.max_bytes, level, (int)k, S.recs, S.rec_stride, Lo.seq_off, Lo.lit_off, Lo.tab_off);
        hipLaunchKernelGGL(lzh_zstd_dfast_entropy_ragged_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes,
                           B.max_bytes, level, (int)k, S.recs, S.rec_stride, Lo.seq_off, Lo.lit_off, Lo.att_off,
                           Lo.tmp_off, S.stage, S.stride, csizes);
    }
    return hipGetLastError();
}

// The entropy stage of block 0 alone, for a caller with a match kernel of its own that writes this kernel's scratch
// layout (zstd_dfast_dict_hip.hip): frames of one block, the parameters the body reads (block size, literal
// compression) being those of the plain call.
hipError_t lzh_launch_zstd_dfast_entropy_ragged(const LzhBatch& B, int level, const LzhSlots& S, uint32_t* csizes,
                                                uint64_t seq_off, uint64_t lit_off, uint64_t att_off, uint64_t tmp_off,
                                                hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_zstd_dfast_entropy_ragged_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes, B.max_bytes,
                       level, 0, S.recs, S.rec_stride, seq_off, lit_off, att_off, tmp_off, S.stage, S.stride, csizes);
    return hipGetLastError();
}

hipError_t lzh_launch_zstd_dfast_compact(const LzhBatch& B, int level, const LzhCompactSlots& S, uint32_t* csizes,
                                         hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    Layout Lo;
    uint32_t nblocks;
    if (!dfast_ragged_geo(B.max_bytes, level, Lo, nblocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lzh_zstd_dfast_compact_slots_kernel, dim3((B.nchunks + 255) / 256), dim3(256), 0, s, B.bytes,
                       B.max_bytes, S.L.stage_sz, S.L.rec_sz, B.nchunks);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = lzh_launch_compact_scans(S.L, B.nchunks, s);
    if (e != hipSuccess) return e;
    for (uint32_t k = 0; k < std::max(nblocks, 1u); k++) {
        hipLaunchKernelGGL(lzh_zstd_dfast_match_compact_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes,
                           B.max_bytes, level, (int)k, S.recs, S.L);
        hipLaunchKernelGGL(lzh_zstd_dfast_entropy_compact_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes,
                           B.max_bytes, level, (int)k, S.recs, S.stage, csizes, S.L);
    }
    return hipGetLastError();
}
