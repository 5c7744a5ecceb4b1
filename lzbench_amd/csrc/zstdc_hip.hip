// lzbench_amd/csrc/zstdc_hip.hip -- zstd 1.5.2 frame compression for gfx950 (the hip_zstd row), bit-exact with the
// reference build for the fast-strategy levels lzbench's zstd rows use.
//
// The uniform kernels (one buffer cut at a chunk size), their launcher, the sizing functions and the debug exports.
// The device code -- the match finder, zc, and the entropy stage, ze -- is in zstdc.h, where the design is described.
#define LZH_TU_VAR   // (the tables and the debug buffer external in this object, as they were when the code stood here)
#include "zstdc.h"

// one wave per frame; block k of every frame
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_match_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size, int level,
                      int k, uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off, uint64_t tab_off,
                      uint32_t lds_arg, uint32_t f0) {
    extern __shared__ __attribute__((aligned(16))) uint32_t zlds[];
    const int lane = threadIdx.x;
    const uint64_t f = (uint64_t)blockIdx.x + f0;   // (f0: the launch's first frame)
    const uint64_t ioff = f * chunk_size;
    if (ioff >= n_total && !(n_total == 0 && f == 0)) return;
    const uint64_t nf = n_total ? min(chunk_size, n_total - ioff) : 0;
#include "zstdc_match_body.inc"
}

// one wave per frame; block k of every frame: entropy coding, block decision, frame assembly
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_entropy_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size, int level, int k,
                        uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off, uint64_t att_off,
                        uint64_t tmp_off, uint8_t* stage, uint64_t stride, uint32_t* csizes, uint32_t f0) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(sizeof(ze::Lds) + 3) / 4];
    LDSA ze::Lds& L = *(LDSA ze::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t f = (uint64_t)blockIdx.x + f0;
    const uint64_t ioff = f * chunk_size;
    if (ioff >= n_total && !(n_total == 0 && f == 0)) return;
    const uint64_t nf = n_total ? min(chunk_size, n_total - ioff) : 0;
#include "zstdc_entropy_body.inc"
}

#include "launch.h"
#include <algorithm>

#if LZH_ZSTDC_STATS
extern "C" int lzh_debug_zstdc_stats(unsigned long long* host, int reset) {
    if (reset) {
        unsigned long long z[24] = {};
        return hipMemcpyToSymbol(HIP_SYMBOL(zc::lzh_zstdc_stats_buf), z, sizeof(z)) == hipSuccess ? 0 : -1;
    }
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(zc::lzh_zstdc_stats_buf), 24 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

size_t lzh_zstd_scratch_stride(size_t chunk_size, int level) {
    const ZParams P = params_for(level, chunk_size);
    if (!P.ok) return 0;
    // the tail chunk may use a larger table (smaller chunks select other clevels rows)
    uint32_t hmax = P.hlog;
    for (int lg = 6; lg <= 31 && (1ull << (lg - 1)) < chunk_size; lg++) {
        const ZParams Q = params_for(level, std::min<uint64_t>(chunk_size, 1ull << lg));
        if (Q.ok) hmax = std::max(hmax, Q.hlog);
    }
    const ZParams T = params_for(level, 1);
    if (T.ok) hmax = std::max(hmax, T.hlog);
    return (size_t)layout_for(P.bsize, hmax).stride;
}

int lzh_zstd_level_ok(int level, size_t chunk_size) {
    // every chunk size up to chunk_size must map to a fast-strategy row
    for (uint64_t n : {(uint64_t)chunk_size, (uint64_t)16384, (uint64_t)131072, (uint64_t)262144, (uint64_t)1})
        if (n <= chunk_size && !params_for(level, n).ok) return 0;
    return 1;
}

// the split of single-block frames over the side stream (0: every launch on the caller's stream)
static int g_zstdc_split = 1;
extern "C" int lzh_debug_zstdc_split(int on) {
    g_zstdc_split = on ? 1 : 0;
    return 0;
}

#ifndef LZH_ZSTD_LDS_MAX
#define LZH_ZSTD_LDS_MAX 65536u   // largest hash table kept in LDS (else in the frame's scratch, via L2)
#endif
// the match kernels' dynamic LDS for frames of up to chunk_size bytes: the hash table of that size's parameters
// (0: it lives in the frame's scratch); the kernels pick the table kind from chunk_size and this
uint32_t lzh_zstd_lds_table(int level, uint64_t chunk_size) {
    const ZParams PF = params_for(level, chunk_size);
    // 3-byte entries (LdsTab24) below 16 MiB chunks, else 4-byte ones
    // (17-bit entries, LdsTab17, for chunks of at most 128 KiB)
    const uint32_t ebytes = chunk_size < (16u << 20) ? 3u : 4u;
    const uint32_t t17 = (2u << PF.hlog) + std::max((1u << PF.hlog) / 8u, 4u);
    return (4u << PF.hlog) > (uint32_t)LZH_ZSTD_LDS_MAX ? 0u
           : chunk_size <= 131072u ? ((t17 + 15u) & ~15u) : (ebytes << PF.hlog);
}

hipError_t lzh_launch_zstd_compress(const LzhInput& I, int level, const LzhSlots& S, uint32_t* csizes, hipStream_t s) {
    const uint32_t nchunks = I.nchunks;
    if (nchunks == 0) return hipSuccess;
    const ZParams P = params_for(level, std::min<uint64_t>(I.chunk_size, I.n_total ? I.n_total : 0));
    if (!P.ok) return hipErrorInvalidValue;
    const ZParams PF = params_for(level, I.chunk_size);
    // the scratch areas are this level's stride apart: S.rec_stride, the layout's largest stride of any level, is here
    // (and nowhere else) an upper bound and not the stride in use -- of the scratch, only S.recs is read
    const size_t fstride = lzh_zstd_scratch_stride(I.chunk_size, level);
    const Layout Lo = layout_for(PF.bsize, 16);   // offsets below tab_off do not depend on hlog
    const uint32_t nblocks =
        (uint32_t)((std::min<uint64_t>(I.chunk_size, std::max<uint64_t>(I.n_total, 1)) + PF.bsize - 1) / PF.bsize);
    const uint32_t lds_tab = lzh_zstd_lds_table(level, I.chunk_size);
    auto match = [&](hipStream_t st, uint32_t k, uint32_t f0, uint32_t nf) {
        hipLaunchKernelGGL(lzh_zstd_match_kernel, dim3(nf), dim3(64), lds_tab, st, I.in, I.n_total, I.in_readable,
                           I.chunk_size, level, (int)k, S.recs, (uint64_t)fstride, Lo.seq_off, Lo.lit_off, Lo.tab_off,
                           lds_tab, f0);
    };
    auto entropy = [&](hipStream_t st, uint32_t k, uint32_t f0, uint32_t nf) {
        hipLaunchKernelGGL(lzh_zstd_entropy_kernel, dim3(nf), dim3(64), 0, st, I.in, I.n_total, I.in_readable,
                           I.chunk_size, level, (int)k, S.recs, (uint64_t)fstride, Lo.seq_off, Lo.lit_off, Lo.att_off,
                           Lo.tmp_off, S.stage, S.stride, csizes, f0);
    };
    // Single-block frames: a frame's entropy stage needs only its own match stage, so the frames split in
    // two.  The first half runs match + entropy on the caller stream's high-priority side stream (its waves go
    // out first), the second half's match on the caller's stream beside it; the first half's entropy then
    // runs beside the second half's matching and only the second half's entropy is left at the end.
    hipStream_t sq = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    if (g_zstdc_split && std::max(nblocks, 1u) == 1 && nchunks >= 2 && lzh_side_stream(s, sq, fork, join)) {
        const uint32_t h = nchunks / 2;
        (void)hipEventRecord(fork, s);
        (void)hipStreamWaitEvent(sq, fork, 0);
        match(sq, 0, 0, h);
        match(s, 0, h, nchunks - h);
        entropy(sq, 0, 0, h);
        (void)hipEventRecord(join, sq);
        entropy(s, 0, h, nchunks - h);
        (void)hipStreamWaitEvent(s, join, 0);
        return hipGetLastError();
    }
    for (uint32_t k = 0; k < std::max(nblocks, 1u); k++) {
        match(s, k, 0, nchunks);
        entropy(s, k, 0, nchunks);
    }
    return hipGetLastError();
}
