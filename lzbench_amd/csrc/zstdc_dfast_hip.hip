// lzbench_amd/csrc/zstdc_dfast_hip.hip -- zstd 1.5.2 frame compression at level 3 for gfx950 (LZH_CODEC_ZSTD_DFAST,
// the hip_zstd_dfast row): the double-fast strategy, bit-exact with the reference build.  Level 3 is ZSTD_dfast in
// all four source-size tables of clevels.h, so every chunk of a batch, the tail included, takes this path.
//
// A frame is processed block by block like the fast-strategy frames of zstdc_hip.hip, each block by two kernels:
//
//   lzh_zstd_dfast_match_kernel    one wave per frame: ZSTD_compressBlock_doubleFast_noDict_generic
//                                  (zstd_double_fast.c:51-253) on the block; sequences + literals to the frame's
//                                  scratch, the same FrameHdr contract as lzh_zstd_match_kernel.
//   lzh_zstd_dfast_entropy_kernel  zstdc_entropy_body.inc with the level-3 window, block size and literal
//                                  compression on: everything after the match finder is shared by fast and
//                                  double-fast (strategy < ZSTD_lazy), so the body is the fast levels' as it is;
//                                  the one strategy-dependent constant, ZSTD_selectEncodingType's 10 - strategy,
//                                  is LZH_ZSTD_STRATEGY 2 of zstdc_dfast.h.
//
// The uniform kernels, their launcher and the sizing function.  The device code -- the entropy stage of zstdc.h for
// ZSTD_dfast, the parser and zdf::WaveEnv -- comes with zstdc_dfast.h, where the match finder is described; nothing
// here changes the fast levels' kernels.
#include "zstdc_dfast.h"

// one wave per frame; block k of every frame
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_dfast_match_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size, int level,
                            int k, uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off,
                            uint64_t tab_off) {
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint64_t ioff = f * chunk_size;
    if (ioff >= n_total && !(n_total == 0 && f == 0)) return;
    const uint64_t nf = n_total ? min(chunk_size, n_total - ioff) : 0;
#include "zstdc_dfast_match_body.inc"
}

// one wave per frame; block k of every frame: the fast levels' entropy stage with the level-3 parameters
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_dfast_entropy_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size, int level,
                              int k, uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off,
                              uint64_t att_off, uint64_t tmp_off, uint8_t* stage, uint64_t stride, uint32_t* csizes) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(sizeof(ze::Lds) + 3) / 4];
    LDSA ze::Lds& L = *(LDSA ze::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint64_t ioff = f * chunk_size;
    if (ioff >= n_total && !(n_total == 0 && f == 0)) return;
    const uint64_t nf = n_total ? min(chunk_size, n_total - ioff) : 0;
    // (the body asks params_for(level, nf) for the frame's parameters: here that name is the level-3 row)
    const auto params_for = [](int lv, uint64_t n) { return zdf::entropy_params(lv, n); };
#include "zstdc_entropy_body.inc"
}

#include <algorithm>
#include "launch.h"

size_t lzh_zstd_dfast_scratch_stride(size_t chunk_size) {
    const zdf::DParams P = zdf::params_for(3, chunk_size);
    // the tail chunk may use other tables (smaller chunks select other clevels rows): the largest of each
    uint32_t hmax = P.hlog, cmax = P.clog;
    for (int lg = 6; lg <= 31 && (1ull << (lg - 1)) < chunk_size; lg++) {
        const zdf::DParams Q = zdf::params_for(3, std::min<uint64_t>(chunk_size, 1ull << lg));
        hmax = std::max(hmax, Q.hlog);
        cmax = std::max(cmax, Q.clog);
    }
    const zdf::DParams T = zdf::params_for(3, 1);
    hmax = std::max(hmax, T.hlog);
    cmax = std::max(cmax, T.clog);
    const Layout Lo = layout_for(P.bsize, 16);   // offsets below tab_off do not depend on hlog
    return (size_t)((Lo.tab_off + (4ull << hmax) + (4ull << cmax) + 255) & ~255ull);
}

hipError_t lzh_launch_zstd_dfast_compress(const LzhInput& I, int level, const LzhSlots& S, uint32_t* csizes,
                                          hipStream_t s) {
    if (I.nchunks == 0) return hipSuccess;
    const zdf::DParams PF = zdf::params_for(level, I.chunk_size);
    if (!PF.ok) return hipErrorInvalidValue;
    // (the stride computed here, as in lzh_launch_zstd_compress; this codec's layout has the one level, so
    // S.rec_stride is the same number)
    const uint64_t fstride = lzh_zstd_dfast_scratch_stride(I.chunk_size);
    const Layout Lo = layout_for(PF.bsize, 16);
    const uint32_t nblocks =
        (uint32_t)((std::min<uint64_t>(I.chunk_size, std::max<uint64_t>(I.n_total, 1)) + PF.bsize - 1) / PF.bsize);
    for (uint32_t k = 0; k < std::max(nblocks, 1u); k++) {
        hipLaunchKernelGGL(lzh_zstd_dfast_match_kernel, dim3(I.nchunks), dim3(64), 0, s, I.in, I.n_total, I.in_readable,
                           I.chunk_size, level, (int)k, S.recs, fstride, Lo.seq_off, Lo.lit_off, Lo.tab_off);
        hipLaunchKernelGGL(lzh_zstd_dfast_entropy_kernel, dim3(I.nchunks), dim3(64), 0, s, I.in, I.n_total,
                           I.in_readable, I.chunk_size, level, (int)k, S.recs, fstride, Lo.seq_off, Lo.lit_off,
                           Lo.att_off, Lo.tmp_off, S.stage, S.stride, csizes);
    }
    return hipGetLastError();
}
