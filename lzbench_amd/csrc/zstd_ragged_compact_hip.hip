// lzbench_amd/csrc/zstd_ragged_compact_hip.hip -- the compact compress layout of ragged zstd batches
// (include/lzbench_hip.h 3c, lzh_zstd_compress_ragged_compact_async): the entry points of zstd_ragged_hip.hip with
// every chunk's staging slot and scratch slot sized from the chunk's own size and level (zstd_ragged_slots.h) and
// placed by an exclusive scan, so a batch's temp grows with its total bytes and not with nchunks x the slots of
// its largest chunk.
//
//   lzh_zstd_compact_slots_kernel   chunk i's two slot sizes (u32; 0 for a chunk over max_bytes)
//   lzh_launch_scan (twice)         the slots' offsets inside the staging region and the scratch region
//   match / entropy per block       as in zstd_ragged_hip.hip, slots reached through those offsets and sizes
//   pack                            lzh_pack_compact_kernel (ragged_compact_hip.hip), the layout's record fields
//                                   carrying the scratch slots
//
// A chunk is processed exactly when its size is at most max_bytes and both of its slots end inside their
// regions (compact_span, ragged_slots.h; the host sizes the regions for the promised total, api.cpp).  Any other chunk is
// handled as an oversize chunk of zstd_ragged_hip.hip: csizes[i] = 0, no packed bytes, no kernel touches a slot.
//
// The kernel bodies are the uniform kernels' text (zstdc_match_body.inc, zstdc_entropy_body.inc), unchanged.  They
// name a frame's scratch `scratch + f * fstride`, its staging slot `stage + f * stride` of `stride` bytes, and
// the areas inside the scratch by seq_off .. tab_off.  Here fstride and stride are ZstdSlot values (a CompactSlot of ragged_slots.h) -- f * slot is the
// slot's scanned offset, the slot converted to an integer its own size -- and the five offsets are locals laid
// out for the chunk's own parameters (lzh_zslot_layout: the layout whose stride is the slot's size), where the
// uniform-slot kernels get them as arguments computed for max_bytes.  Every buffer descriptor the bodies build is
// therefore bounded by the chunk's own slot.  chunk_size (the batch's max_bytes) and lds_arg still select the
// hash-table kind alone: speed, never bytes.
// As in zstd_ragged_hip.hip, the device functions are those of zstdc.h, compiled with the flags of zstdc_hip.hip.
#include "zstdc.h"
#include "zstd_ragged_slots.h"

// (ZstdSlot: ragged_slots.h)
// -------------------------------------------------------------------------------------- slot sizes
extern "C" __global__ void __launch_bounds__(256)
lzh_zstd_compact_slots_kernel(const uint64_t* in_bytes, uint64_t max_bytes, int level, uint32_t* stage_sz,
                              uint32_t* scratch_sz, uint32_t nchunks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchunks) return;
    const uint64_t b = in_bytes[i];
    const bool over = b > max_bytes;
    stage_sz[i] = over ? 0u : (uint32_t)lzh_zslot_stage_bytes(b);
    scratch_sz[i] = over ? 0u : (uint32_t)lzh_zslot_scratch_bytes(level, b);
}

// ---------------------------------------------------------------------------- match and entropy
// one wave per chunk; block k of every chunk (a chunk of fewer blocks returns at once)
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_match_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level, int k,
                              uint8_t* scratch, uint32_t lds_arg, const LzhCompactLayout C) {
    extern __shared__ __attribute__((aligned(16))) uint32_t zlds[];
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint64_t chunk_size = max_bytes;
    const uint64_t ioff = 0;
    const uint8_t* in;
    int sn;
    ZstdSlot stride, fstride;
    if (!compact_span(in_ptrs, in_bytes, f, max_bytes, C, in, sn, stride, fstride)) return;
    const uint64_t nf = (uint64_t)sn;
    const uint64_t in_readable = nf + 16;
    const Layout Lo = lzh_zslot_layout(lzh_zslot_params(level, nf));
    const uint64_t seq_off = Lo.seq_off, lit_off = Lo.lit_off, tab_off = Lo.tab_off;
#include "zstdc_match_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_entropy_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level,
                                int k, uint8_t* scratch, uint8_t* stage, uint32_t* csizes, const LzhCompactLayout C) {
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
    const Layout Lo = lzh_zslot_layout(lzh_zslot_params(level, nf));
    const uint64_t seq_off = Lo.seq_off, lit_off = Lo.lit_off, att_off = Lo.att_off, tmp_off = Lo.tmp_off;
#include "zstdc_entropy_body.inc"
}

// ------------------------------------------------------------------------- host side: arithmetic, launcher
#include <algorithm>

LzhCompactRegions lzh_zstd_compact_regions(int level, uint64_t total, uint64_t max_bytes, uint64_t nchunks) {
    return lzh_zslot_regions(level, total, max_bytes, nchunks);
}

LzhCompactRegions lzh_zstd_compact_slot(int level, uint64_t n) {
    return {lzh_zslot_stage_bytes(n), lzh_zslot_scratch_bytes(level, n)};
}

hipError_t lzh_launch_zstd_compact(const LzhBatch& B, int level, const LzhCompactSlots& S, uint32_t* csizes,
                                   hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    // (the block count and the table's LDS of a batch of empty chunks are those of 1-byte chunks, as in
    // lzh_launch_zstd_ragged)
    const uint64_t geo = std::max<uint64_t>(B.max_bytes, 1);
    const ZParams PF = params_for(level, geo);
    if (!PF.ok) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lzh_zstd_compact_slots_kernel, dim3((B.nchunks + 255) / 256), dim3(256), 0, s, B.bytes,
                       B.max_bytes, level, S.L.stage_sz, S.L.rec_sz, B.nchunks);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = lzh_launch_compact_scans(S.L, B.nchunks, s);
    if (e != hipSuccess) return e;
    const uint32_t nblocks = (uint32_t)((geo + PF.bsize - 1) / PF.bsize);
    const uint32_t lds_tab = lzh_zstd_lds_table(level, geo);
    // (every launch on s, as lzh_launch_zstd_ragged: a captured call has no parallel branches)
    for (uint32_t k = 0; k < std::max(nblocks, 1u); k++) {
        hipLaunchKernelGGL(lzh_zstd_match_compact_kernel, dim3(B.nchunks), dim3(64), lds_tab, s, B.ptrs, B.bytes,
                           B.max_bytes, level, (int)k, S.recs, lds_tab, S.L);
        hipLaunchKernelGGL(lzh_zstd_entropy_compact_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes, B.max_bytes,
                           level, (int)k, S.recs, S.stage, csizes, S.L);
    }
    return hipGetLastError();
}
