// lzbench_amd/csrc/zstd_dfast_dict_hip.hip -- ragged zstd level-3 batches with a shared raw-content dictionary
// (include/lzbench_hip.h 3h): frame i is what zstd 1.5.2 writes for ZSTD_compress_usingDict(chunk i, dictionary, 3)
// with the dictionary in a buffer of its own; it decodes with 3f's lzh_zstd_decompress_ragged_dict_async.
//
//   lzh_zstd_dfast_dict_zero_kernel, lzh_zstd_dfast_dict_table_kernel    once per call:
//                                    ZSTD_fillDoubleHashTable(ZSTD_dtlm_fast) over the dictionary, one filled pair of
//                                    tables per (hashLog, chainLog, minMatch) class a batch can take
//                                    (zfd::classes_for; a frame's class follows from its own size).  An entry is the
//                                    largest inserted index of its bucket, so the fill is a max-reduction in any order.
//   lzh_zstd_dfast_dict_match_kernel one wave per chunk: zeroes a private pair of tables in the frame's scratch, then
//                                    runs ZSTD_compressBlock_doubleFast_extDict_generic (zfd::ext_block,
//                                    zstd_dfast_dict_parse.h) with wave-uniform state.  A lookup reads the private entry
//                                    and the class's shared filled entry together and takes the shared one where the
//                                    private one is 0: every chunk index is nonzero and a chunk's put always replaces
//                                    the dictionary's entry, so this is the table a private copy would hold, without
//                                    the copy's reads.  The dictionary is read in place below prefixStartIndex, the
//                                    chunk above it; forward and backward counts run over the 64 lanes.  Sequences and
//                                    literals go to the scratch layout lzh_zstd_dfast_entropy_ragged_kernel reads
//                                    (zstd_dfast_ragged_hip.hip), which then writes the frame: with one block per frame
//                                    and a single-segment header nothing after the match finder depends on the
//                                    dictionary.
//
// The device functions are those of zstdc_dfast.h (and through it of zstdc.h); no existing kernel's code changes.  What
// the match kernel and its launcher share with level 1's (zstd_dict_hip.hip) is zstd_dict_env.h.
#include "zstdc_dfast.h"
#include "zstd_dfast_dict_parse.h"
#include "zstd_dict_env.h"

namespace zfd {

struct ClassArg {
    uint32_t count;
    uint32_t hlog[kClassCountMax], clog[kClassCountMax], mls[kClassCountMax], off[kClassCountMax];
};

// ext_block's environment on one wave: zde::WaveBytes, 64-bit reads of the chunk and of the dictionary, and the private
// pair of tables in the frame's scratch (L, S) over the class's shared filled pair (LD, SD)
struct WaveEnv : zde::WaveBytes {
    zc::GlbTab L, S;
    rsrc_t LD, SD;
    __device__ __forceinline__ uint64_t r64(int p) const {
        return p >= 0 ? uni64(zc::ld64(in, p)) : uni64(zc::ld64(dict, max(D + p, 0)));
    }
    // (both loads are issued before either is used; h < 1 << log of both tables of the pair: inside their descriptors)
    __device__ __forceinline__ uint32_t long_get(uint32_t h) const {
        const uint32_t own = L.get(h), filled = ld_b32(LD, (int)(h * 4));
        return uni(own ? own : filled);
    }
    __device__ __forceinline__ uint32_t short_get(uint32_t h) const {
        const uint32_t own = S.get(h), filled = ld_b32(SD, (int)(h * 4));
        return uni(own ? own : filled);
    }
    __device__ __forceinline__ void long_put(uint32_t h, uint32_t v) const { if (lane == 0) L.put(h, v); }
    __device__ __forceinline__ void short_put(uint32_t h, uint32_t v) const { if (lane == 0) S.put(h, v); }
    __device__ __forceinline__ void fence() const { L.fence(); }
    __device__ __forceinline__ void event(int) const {}
};

}  // namespace zfd

// the table region starts empty (a kernel, not a memset: a captured call stays a chain of kernel nodes)
extern "C" __global__ void __launch_bounds__(256)
lzh_zstd_dfast_dict_zero_kernel(uint32_t* tables, uint32_t ndwords) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < ndwords) tables[i] = 0u;
}

// one thread per inserted dictionary position (0, 3, 6, ..), blockIdx.y = the class: both tables of its pair
extern "C" __global__ void __launch_bounds__(256)
lzh_zstd_dfast_dict_table_kernel(const uint8_t* dict, uint32_t dict_bytes, uint32_t nfill, uint32_t* tables,
                                 const zfd::ClassArg C) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const uint32_t c = blockIdx.y;
    if (q >= nfill || c >= C.count) return;
    Bytes d;
    d.init(dict, (uint64_t)dict_bytes + 16);
    const uint64_t v = zc::ld64(d, (int)(3u * q));
    // (a hash is below 1 << its log: inside its table; the short table follows the long one)
    uint32_t* lt = tables + C.off[c] / 4;
    atomicMax(lt + zdf::hash8(v, C.hlog[c]), 2u + 3u * q);
    atomicMax(lt + (1u << C.hlog[c]) + zdf::hash_short(v, C.clog[c], C.mls[c]), 2u + 3u * q);
}

// one wave per chunk: the frame's one block
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_dfast_dict_match_kernel(const uint8_t* dict, uint32_t dict_bytes, const uint8_t* tables, const zfd::ClassArg C,
                                 const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level,
                                 uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off,
                                 uint64_t tab_off, uint32_t tab_cap) {
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint8_t* in;
    int sn;
    if (!ragged_span(in_ptrs, in_bytes, f, max_bytes, in, sn)) return;
    uint8_t* fs = scratch + f * fstride;
    rsrc_t hdr = make_rsrc(fs, 64);
    const zfd::XParams P = zfd::params_for(level, (uint64_t)sn, dict_bytes);
    uint32_t toff = ~0u;
    for (uint32_t c = 0; c < C.count; c++)
        if (C.hlog[c] == P.hlog && C.clog[c] == P.clog && C.mls[c] == P.mls) toff = C.off[c];
    const uint32_t lbytes = 4u << P.hlog, sbytes = 4u << P.clog;
    if (sn < 7 || !P.ok || toff == ~0u || lbytes + sbytes > tab_cap) {   // ZSTD_buildSeqStore: too small, stored raw
        zde::raw_header(hdr, lane);
        return;
    }
    // the frame's private pair starts empty (16 bytes a lane; tab_off is 256-aligned, both sizes multiples of 256)
    rsrc_t both = make_rsrc(fs + tab_off, lbytes + sbytes);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (uint32_t o = 16u * lane; o < lbytes + sbytes; o += 16u * LZH_WAVE)
        __builtin_amdgcn_raw_buffer_store_b128(zero, both, (int)o, 0, 0);
    Bytes in_b, dict_b;
    in_b.init(in, (uint64_t)sn + 16);
    dict_b.init(dict, (uint64_t)dict_bytes + 16);
    SeqOut O;
    zde::seq_store(O, fs, seq_off, lit_off, P.bsize);
    uint32_t rep[2] = {1u, 4u};                          // repStartValue
    zfd::WaveEnv E{{in_b, dict_b, (int)dict_bytes, O, lane},
                   GlbTab{make_rsrc(fs + tab_off, lbytes)}, GlbTab{make_rsrc(fs + tab_off + lbytes, sbytes)},
                   make_rsrc(tables + toff, lbytes), make_rsrc(tables + toff + lbytes, sbytes)};
    E.fence();
    const int anchor = zfd::ext_block(E, P, dict_bytes, sn, rep);
    zde::close_frame(hdr, in_b, O, anchor, sn, rep, lane);
}

// ------------------------------------------------------------------------- host side: arithmetic, launchers
#include <algorithm>
#include <vector>
#include "launch.h"

// the largest pair of tables of any frame of a batch: hashLog never passes log2(n + dict_bytes) + 1 nor 16, chainLog
// never log2(n + dict_bytes) nor 16; monotone in both sizes (the batch's own classes are not: a larger dictionary can
// drop the small tables)
static uint32_t dfast_dict_pair_cap(uint64_t dict_bytes, uint64_t max_bytes) {
    const uint32_t lg = zde::total_log(dict_bytes, max_bytes);
    return (4u << std::min(16u, lg + 1)) + (4u << std::min(16u, lg));
}

size_t lzh_zstd_dfast_dict_scratch_stride(size_t dict_bytes, size_t max_bytes) {
    const Layout Lo = layout_for((uint32_t)std::max<size_t>(max_bytes, 1), 6);   // offsets below tab_off do not depend on hlog
    return (size_t)((Lo.tab_off + dfast_dict_pair_cap(dict_bytes, max_bytes) + 255) & ~255ull);
}

size_t lzh_zstd_dfast_dict_tables_bytes(void) { return (zfd::kClassBytesMax + 255u) & ~255u; }

int lzh_zstd_dfast_dict_params(int level, uint64_t n, uint64_t dict_bytes, uint32_t* out) {
    const zfd::XParams P = zfd::params_for(level, n, dict_bytes);
    if (!P.ok) return 0;
    out[0] = P.wlog;
    out[1] = P.hlog;
    out[2] = P.clog;
    out[3] = P.mls;
    out[4] = std::min(1u << P.wlog, 131072u);
    return 1;
}

long lzh_zstd_dfast_dict_host_parse(int level, const uint8_t* dict, uint64_t dict_bytes, const uint8_t* src, uint64_t n,
                                    uint32_t* seqs, uint64_t cap, uint64_t* events) {
    std::vector<uint32_t> tab(2u << 16);
    return zfd::host_walk(level, dict, dict_bytes, src, n, seqs, cap, tab.data(), events);
}

hipError_t lzh_launch_zstd_dfast_dict(const uint8_t* dict, uint32_t dict_bytes, uint8_t* tables, const LzhBatch& B,
                                      int level, const LzhSlots& S, uint32_t* csizes, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    const uint64_t max_bytes = B.max_bytes;
    if (!zfd::level_ok(level) || dict_bytes < zfd::kDictMin || dict_bytes > zfd::kDictMax || max_bytes > zfd::kChunkMax)
        return hipErrorInvalidValue;
    const zfd::Classes K = zfd::classes_for(level, dict_bytes, max_bytes);
    if (K.count > zfd::kClassCountMax || K.bytes > lzh_zstd_dfast_dict_tables_bytes()) return hipErrorInvalidValue;
    if (S.rec_stride < lzh_zstd_dfast_dict_scratch_stride(dict_bytes, max_bytes)) return hipErrorInvalidValue;
    zfd::ClassArg C{};
    zde::fill_class_arg(C, K);
    for (uint32_t i = 0; i < K.count; i++) C.clog[i] = K.clog[i];
    const Layout Lo = layout_for((uint32_t)std::max<uint64_t>(max_bytes, 1), 6);
    const hipError_t e = zde::launch_chain(lzh_zstd_dfast_dict_zero_kernel, lzh_zstd_dfast_dict_table_kernel,
                                           lzh_zstd_dfast_dict_match_kernel, C, K.bytes, zdd::fill_count(dict_bytes), dict,
                                           dict_bytes, tables, B, level, S, Lo,
                                           dfast_dict_pair_cap(dict_bytes, max_bytes), s);
    if (e != hipSuccess) return e;
    return lzh_launch_zstd_dfast_entropy_ragged(B, level, S, csizes, Lo.seq_off, Lo.lit_off, Lo.att_off, Lo.tmp_off, s);
}
