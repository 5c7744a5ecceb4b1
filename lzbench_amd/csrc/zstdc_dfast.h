// lzbench_amd/csrc/zstdc_dfast.h -- device code of the zstd level-3 (double-fast) compressor: the entropy stage of
// zstdc.h compiled for ZSTD_dfast, the parser (zstd_dfast_parse.h) and its environment on one wave (namespace zdf, with
// zstdc_dfast_match_body.inc).  Included by zstdc_dfast_hip.hip (the uniform kernels) and zstd_dfast_ragged_hip.hip;
// no kernel is defined here.
//
// The match finder walks position by position (zstd_dfast_parse.h); the wave shares each position's loads,
// counts match lengths 256 bytes a round and copies literals 64..256 bytes a round (count_fwd, count_bwd,
// lit_copy of zstdc.h).  The two tables (long: 4 << hashLog, short: 4 << chainLog bytes, up to 768 KiB a
// frame) live in the frame's scratch after the fast levels' areas and are served from L2; they start zeroed per
// frame and persist across its blocks.  A table store becomes visible to the wave's later loads through a wait
// for it (GlbTab::fence) and loads that bypass L1, as in the fast levels' scratch table.
#pragma once
// The strategy must be defined before a unit first sees zstdc.h, which otherwise takes ZSTD_fast (1): the order of the
// two lines below sees to that, as long as the unit has not included zstdc.h itself before this header.
#ifdef LZH_ZSTD_STRATEGY_DEFAULTED
#error "zstdc_dfast.h must come before zstdc.h: the entropy stage has already been compiled for LZH_ZSTD_STRATEGY 1"
#endif
#define LZH_ZSTD_STRATEGY 2   // ZSTD_dfast: ZSTD_selectEncodingType's thresholds (the one place the stage reads it)
#include "zstdc.h"
#include "zstd_dfast_parse.h"

namespace zdf {

// the level-3 parameters in the shape the entropy body reads (window, block size, literal compression on)
__host__ __device__ inline zc::ZParams entropy_params(int level, uint64_t n) {
    const DParams D = params_for(level, n);
    zc::ZParams p{};
    p.ok = D.ok;
    p.wlog = D.wlog;
    p.hlog = D.hlog;
    p.mls = D.mls;
    p.step = 2;
    p.bsize = D.bsize;
    p.lit_off = 0;                      // double-fast never disables literal compression
    return p;
}

// dfast_block's environment on one wave: uniform loads of the frame, the two tables in the frame's scratch
struct WaveEnv {
    const Bytes& in;
    zc::GlbTab L, S;
    zc::SeqOut& O;
    int lane;
    __device__ __forceinline__ uint32_t r32(int pos) const { return uni(in.w32(max(pos, 0))); }
    __device__ __forceinline__ uint64_t r64(int pos) const { return uni64(zc::ld64(in, max(pos, 0))); }
    __device__ __forceinline__ int count_fwd(int a, int b, int maxn) const { return zc::count_fwd(in, a, b, maxn, lane); }
    __device__ __forceinline__ int count_bwd(int a, int b, int maxn) const { return zc::count_bwd(in, a, b, maxn, lane); }
    __device__ __forceinline__ uint32_t long_get(uint32_t h) const { return uni(L.get(h)); }
    __device__ __forceinline__ uint32_t short_get(uint32_t h) const { return uni(S.get(h)); }
    __device__ __forceinline__ void long_put(uint32_t h, uint32_t v) const { if (lane == 0) L.put(h, v); }
    __device__ __forceinline__ void short_put(uint32_t h, uint32_t v) const { if (lane == 0) S.put(h, v); }
    __device__ __forceinline__ void fence() const { L.fence(); }
    __device__ __forceinline__ void seq(int from, int ll, uint32_t offBase, uint32_t mlen) const {
        zc::lit_copy(in, from, O.lits, O.nl, ll, lane);
        O.nl += ll;
        O.put(lane, (uint32_t)ll, offBase, mlen);
    }
};

}  // namespace zdf
