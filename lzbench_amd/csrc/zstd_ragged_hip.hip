// lzbench_amd/csrc/zstd_ragged_hip.hip -- zstd compression of ragged batches (include/lzbench_hip.h 3c): the
// chunks of a batch are given by device arrays of pointers and sizes, chunk i becomes the frame the uniform call
// writes for a chunk of that size alone.
//
// The two kernels are lzh_zstd_match_kernel and lzh_zstd_entropy_kernel of zstdc_hip.hip with another frame
// lookup: ragged_span (common.h) loads chunk blockIdx.x's pointer and size once and makes them wave-uniform, and
// the body that follows is the uniform kernel's, shared as text (zstdc_match_body.inc, zstdc_entropy_body.inc)
// under the names the uniform kernels use: in + ioff is the frame's address (ioff = 0 here), in_readable - ioff
// the bytes that may be read from it (nf + 16 here), nf its size, chunk_size the batch's max_bytes.  The bodies
// derive the frame's parameters from nf on the device, as they do for a uniform batch's tail chunk; max_bytes only
// selects the hash-table kind (speed, never bytes), sizes the slots and bounds the number of block launches.
// The device functions are those of zstdc.h, compiled here with the flags of zstdc_hip.hip, so every function has
// the one caller per code object that it has in that unit.  Nothing here changes the uniform kernels' code
// (profiles/traffic*.json are keyed to their code hashes).
//
// Frame i's staging slot and scratch area are slot i of the batch's, each sized for max_bytes and reached through
// buffer descriptors of that size or less.  A chunk whose device-side size passes max_bytes is not processed: no
// kernel touches its slots, its compressed size is 0.
#include "zstdc.h"

// one wave per chunk; block k of every chunk (a chunk of fewer blocks returns at once)
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_match_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level, int k,
                             uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off, uint64_t tab_off,
                             uint32_t lds_arg) {
    extern __shared__ __attribute__((aligned(16))) uint32_t zlds[];
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint64_t chunk_size = max_bytes;
    const uint64_t ioff = 0;
    const uint8_t* in;
    int sn;
    if (!ragged_span(in_ptrs, in_bytes, f, max_bytes, in, sn)) return;
    const uint64_t nf = (uint64_t)sn;
    const uint64_t in_readable = nf + 16;
#include "zstdc_match_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_entropy_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level, int k,
                               uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off, uint64_t att_off,
                               uint64_t tmp_off, uint8_t* stage, uint64_t stride, uint32_t* csizes) {
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
#include "zstdc_entropy_body.inc"
}

#include <algorithm>
#include "launch.h"

hipError_t lzh_launch_zstd_ragged(const LzhBatch& B, int level, const LzhSlots& S, uint32_t* csizes, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    // (the slots of a batch of empty chunks are those of 1-byte chunks, as api.cpp sizes them: size 0 is
    // ZSTD_getParams' "unknown size")
    const uint64_t geo = std::max<uint64_t>(B.max_bytes, 1);
    const ZParams PF = params_for(level, geo);
    if (!PF.ok) return hipErrorInvalidValue;
    if (S.rec_stride < lzh_zstd_scratch_stride(geo, level)) return hipErrorInvalidValue;
    const Layout Lo = layout_for(PF.bsize, 16);   // offsets below tab_off do not depend on hlog
    const uint32_t nblocks = (uint32_t)((geo + PF.bsize - 1) / PF.bsize);
    const uint32_t lds_tab = lzh_zstd_lds_table(level, geo);
    // (the uniform launcher's plain loop; its side-stream split of single-block frames is left out on purpose:
    // every launch stays on s, so a captured call has no parallel branches)
    for (uint32_t k = 0; k < std::max(nblocks, 1u); k++) {
        hipLaunchKernelGGL(lzh_zstd_match_ragged_kernel, dim3(B.nchunks), dim3(64), lds_tab, s, B.ptrs, B.bytes,
                           B.max_bytes, level, (int)k, S.recs, S.rec_stride, Lo.seq_off, Lo.lit_off, Lo.tab_off, lds_tab);
        hipLaunchKernelGGL(lzh_zstd_entropy_ragged_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes, B.max_bytes,
                           level, (int)k, S.recs, S.rec_stride, Lo.seq_off, Lo.lit_off, Lo.att_off, Lo.tmp_off, S.stage,
                           S.stride, csizes);
    }
    return hipGetLastError();
}

// The entropy stage of block 0 alone, for a caller with a match kernel of its own that writes this kernel's scratch
// layout (zstd_dict_hip.hip): frames of one block, the parameters the body reads (block size, literal compression)
// being those of the plain call.
hipError_t lzh_launch_zstd_entropy_ragged(const LzhBatch& B, int level, const LzhSlots& S, uint32_t* csizes,
                                          uint64_t seq_off, uint64_t lit_off, uint64_t att_off, uint64_t tmp_off,
                                          hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_zstd_entropy_ragged_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes, B.max_bytes,
                       level, 0, S.recs, S.rec_stride, seq_off, lit_off, att_off, tmp_off, S.stage, S.stride, csizes);
    return hipGetLastError();
}
