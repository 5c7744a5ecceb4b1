// lzbench_amd/csrc/zstd_dict_hip.hip -- ragged zstd batches with a shared raw-content dictionary
// (include/lzbench_hip.h 3f): frame i is what zstd 1.5.2 writes for ZSTD_compress_usingDict(chunk i, dictionary) with
// the dictionary in a buffer of its own, and decodes as ZSTD_decompress_usingDict does.
//
//   lzh_zstd_dict_zero_kernel, lzh_zstd_dict_table_kernel       once per call: ZSTD_fillHashTable(ZSTD_dtlm_fast) over the dictionary, one filled
//                                    table per (hashLog, minMatch) class a batch can take (zdd::classes_for; a frame's
//                                    class follows from its own size).  An entry is the largest inserted index of its
//                                    bucket, so the fill is a max-reduction over lanes and blocks, in any order.
//   lzh_zstd_dict_match_kernel       one wave per chunk: copies its class's table into the frame's scratch (global
//                                    memory, served from L2 like the level-3 tables), then runs
//                                    ZSTD_compressBlock_fast_extDict_generic (zdd::ext_block, zstd_dict_parse.h) with
//                                    wave-uniform state; the dictionary is read in place below prefixStartIndex, the
//                                    chunk above it; forward and backward counts run over the 64 lanes.  Sequences and
//                                    literals go to the scratch layout lzh_zstd_entropy_ragged_kernel reads
//                                    (zstd_ragged_hip.hip), which then writes the frame: with one block per frame and a
//                                    single-segment header nothing after the match finder depends on the dictionary.
//   lzh_zstd_dict_decompress_kernel  lzh_zstd_decompress_ragged_kernel with the dictionary as a second match source
//                                    (zstdd::decode_frame's DictT): an offset may reach dict_bytes before the chunk's
//                                    first byte; such a sequence copies dictionary bytes, then output bytes.
//
// The compressor's device functions are zstdc.h, the decoder's are zstdd.h; neither's kernels change.  What the match
// kernel and its launcher share with level 3's (zstd_dfast_dict_hip.hip) is zstd_dict_env.h.
#include "zstdc.h"
#include "zstdd.h"
#include "zstd_dict_parse.h"
#include "zstd_dict_env.h"

namespace zdd {

struct ClassArg {
    uint32_t count;
    uint32_t hlog[12], mls[12], off[12];
};

// ext_block's environment on one wave: zde::WaveBytes and the table in the scratch; the fast walk's 64-bit reads are of
// the chunk alone
struct WaveEnv : zde::WaveBytes {
    zc::GlbTab T;
    __device__ __forceinline__ uint64_t r64(int p) const { return uni64(zc::ld64(in, max(p, 0))); }
    __device__ __forceinline__ uint32_t get(uint32_t h) const { return uni(T.get(h)); }
    __device__ __forceinline__ void put(uint32_t h, uint32_t v) const { if (lane == 0) T.put(h, v); }
    __device__ __forceinline__ void fence() const { T.fence(); }
};

// the decoder's second match source: the dictionary's last `back` bytes
struct DictSrc {
    static constexpr bool kOn = true;
    Bytes d;
    int bytes;
    // out[pos, pos + n) = the n dictionary bytes that start `back` bytes before the dictionary's end
    __device__ __forceinline__ void copy(zstdd::ZSink& O, int pos, int back, int n, int lane) const {
        for (int base = 0; base < n; base += LZH_WAVE) {
            const int t = base + lane;
            const uint32_t v = d.b(bytes - back + (t < n ? t : 0));
            if (t < n) O.put(pos + t, v);
            O.maybe_flush(pos + min(base + LZH_WAVE, n), lane);
        }
    }
};

}  // namespace zdd

// the table region starts empty (a kernel, not a memset: a captured call stays a chain of kernel nodes)
extern "C" __global__ void __launch_bounds__(256)
lzh_zstd_dict_zero_kernel(uint32_t* tables, uint32_t ndwords) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < ndwords) tables[i] = 0u;
}

// one thread per inserted dictionary position (0, 3, 6, ..), blockIdx.y = the class
extern "C" __global__ void __launch_bounds__(256)
lzh_zstd_dict_table_kernel(const uint8_t* dict, uint32_t dict_bytes, uint32_t nfill, uint32_t* tables,
                           const zdd::ClassArg C) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const uint32_t c = blockIdx.y;
    if (q >= nfill || c >= C.count) return;
    Bytes d;
    d.init(dict, (uint64_t)dict_bytes + 16);
    const uint32_t h = zdd::hashp(zc::ld64(d, (int)(3u * q)), C.hlog[c], C.mls[c]);   // (h < 1 << hlog: inside the table)
    atomicMax(tables + C.off[c] / 4 + h, 2u + 3u * q);
}

// one wave per chunk: the frame's one block
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_dict_match_kernel(const uint8_t* dict, uint32_t dict_bytes, const uint8_t* tables, const zdd::ClassArg C,
                           const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int level,
                           uint8_t* scratch, uint64_t fstride, uint64_t seq_off, uint64_t lit_off, uint64_t tab_off,
                           uint32_t tab_cap) {
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    const uint8_t* in;
    int sn;
    if (!ragged_span(in_ptrs, in_bytes, f, max_bytes, in, sn)) return;
    uint8_t* fs = scratch + f * fstride;
    rsrc_t hdr = make_rsrc(fs, 64);
    const zdd::XParams P = zdd::params_for(level, (uint64_t)sn, dict_bytes);
    uint32_t toff = ~0u;
    for (uint32_t c = 0; c < C.count; c++)
        if (C.hlog[c] == P.hlog && C.mls[c] == P.mls) toff = C.off[c];
    const uint32_t tbytes = 4u << P.hlog;
    if (sn < 7 || !P.ok || toff == ~0u || tbytes > tab_cap) {   // ZSTD_buildSeqStore: too small, stored raw
        zde::raw_header(hdr, lane);
        return;
    }
    // the frame's own copy of its class's table (16 bytes a lane; both sides 256-aligned)
    rsrc_t tsrc = make_rsrc(tables + toff, tbytes), tdst = make_rsrc(fs + tab_off, tbytes);
    for (uint32_t o = 16u * lane; o < tbytes; o += 16u * LZH_WAVE) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(tsrc, (int)o, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(v, tdst, (int)o, 0, 0);
    }
    Bytes in_b, dict_b;
    in_b.init(in, (uint64_t)sn + 16);
    dict_b.init(dict, (uint64_t)dict_bytes + 16);
    SeqOut O;
    zde::seq_store(O, fs, seq_off, lit_off, P.bsize);
    uint32_t rep[2] = {1u, 4u};                          // repStartValue
    zdd::WaveEnv E{{in_b, dict_b, (int)dict_bytes, O, lane}, GlbTab{tdst}};
    E.fence();
    const int anchor = zdd::ext_block(E, P, dict_bytes, sn, rep);
    zde::close_frame(hdr, in_b, O, anchor, sn, rep, lane);
}

extern "C" __global__ void __launch_bounds__(64, LZH_ZSTD_MINW)
lzh_zstd_dict_decompress_kernel(const uint8_t* dict, uint32_t dict_bytes, const uint8_t* packed, uint64_t packed_readable,
                                const uint64_t* offsets, const uint32_t* csizes, void* const* out_ptrs,
                                const uint64_t* out_bytes, uint64_t max_bytes, int32_t* status) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(sizeof(zstdd::Lds) + 3) / 4];
    LDSA zstdd::Lds& L = *(LDSA zstdd::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint8_t* outc;
    int part;
    if (!ragged_span((const void* const*)out_ptrs, out_bytes, chunk, max_bytes, outc, part)) {
        if (lane == 0) status[chunk] = -1;
        return;
    }
    uint8_t* out = (uint8_t*)outc;
    const uint64_t ioff = offsets[chunk];
    const int cs = (int)csizes[chunk];
    // (+16: whole-dword reads of the frame's last bytes; bytes past the frame are never used)
    const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, (uint64_t)cs + 16) : 0;
    Bytes rin, rout;
    rin.init(packed + ioff, readable);
    rout.init(out, (uint64_t)part);
    int r;
    if (cs == part) {                                  // stored raw (the raw-store rule of the compress calls)
        copy_raw(rin, rout, part, lane);
        r = part;
    } else {
        zstdd::ZSink O{(LDSA uint8_t*)L.win, rout, 0, 0};
        for (int i = lane; i < 36 + 53; i += LZH_WAVE) L.base[i] = i < 36 ? zstdd::kLLBase[i] : zstdd::kMLBase[i - 36];
        wave_lds_fence();
        Bytes lout;
        lout.init(out, (uint64_t)part + 3);
        zdd::DictSrc D;
        D.d.init(dict, (uint64_t)dict_bytes);
        D.bytes = (int)dict_bytes;
        r = zstdd::decode_frame(rin, lout, cs, O, L, part, lane, nullptr, D);
        if (r > 0) O.flush(r, lane);
    }
    if (lane == 0) status[chunk] = r;
}

// ------------------------------------------------------------------------- host side: arithmetic, launchers
#include <algorithm>
#include <vector>
#include "launch.h"

// the largest table of any frame of a batch: hashLog never passes log2(n + dict_bytes) + 1, nor the level-1 row's 15;
// monotone in both sizes (the batch's own classes are not: a larger dictionary can drop the small tables)
static uint32_t dict_hlog_cap(uint64_t dict_bytes, uint64_t max_bytes) {
    return std::min(15u, zde::total_log(dict_bytes, max_bytes) + 1);
}

size_t lzh_zstd_dict_scratch_stride(size_t dict_bytes, size_t max_bytes) {
    return (size_t)layout_for((uint32_t)std::max<size_t>(max_bytes, 1), dict_hlog_cap(dict_bytes, max_bytes)).stride;
}

size_t lzh_zstd_dict_tables_bytes(void) { return (zdd::kClassBytesMax + 255u) & ~255u; }

int lzh_zstd_dict_params(int level, uint64_t n, uint64_t dict_bytes, uint32_t* out) {
    const zdd::XParams P = zdd::params_for(level, n, dict_bytes);
    if (!P.ok) return 0;
    out[0] = P.wlog;
    out[1] = P.hlog;
    out[2] = P.mls;
    out[3] = P.tlen;
    out[4] = std::min(1u << P.wlog, 131072u);
    return 1;
}

long lzh_zstd_dict_host_parse(int level, const uint8_t* dict, uint64_t dict_bytes, const uint8_t* src, uint64_t n,
                              uint32_t* seqs, uint64_t cap) {
    std::vector<uint32_t> tab(1u << 15);
    return zdd::host_walk(level, dict, dict_bytes, src, n, seqs, cap, tab.data());
}

hipError_t lzh_launch_zstd_dict(const uint8_t* dict, uint32_t dict_bytes, uint8_t* tables, const LzhBatch& B, int level,
                                const LzhSlots& S, uint32_t* csizes, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    const uint64_t max_bytes = B.max_bytes;
    if (!zdd::level_ok(level) || dict_bytes < zdd::kDictMin || dict_bytes > zdd::kDictMax || max_bytes > zdd::kChunkMax)
        return hipErrorInvalidValue;
    const zdd::Classes K = zdd::classes_for(level, dict_bytes, max_bytes);
    if (K.count > 12 || K.bytes > lzh_zstd_dict_tables_bytes()) return hipErrorInvalidValue;
    if (S.rec_stride < lzh_zstd_dict_scratch_stride(dict_bytes, max_bytes)) return hipErrorInvalidValue;
    zdd::ClassArg C{};
    zde::fill_class_arg(C, K);
    const uint32_t hcap = dict_hlog_cap(dict_bytes, max_bytes);
    const Layout Lo = layout_for((uint32_t)std::max<uint64_t>(max_bytes, 1), hcap);
    const hipError_t e = zde::launch_chain(lzh_zstd_dict_zero_kernel, lzh_zstd_dict_table_kernel, lzh_zstd_dict_match_kernel,
                                           C, K.bytes, zdd::fill_count(dict_bytes), dict, dict_bytes, tables, B, level, S,
                                           Lo, 4u << hcap, s);
    if (e != hipSuccess) return e;
    return lzh_launch_zstd_entropy_ragged(B, level, S, csizes, Lo.seq_off, Lo.lit_off, Lo.att_off, Lo.tmp_off, s);
}

hipError_t lzh_launch_zstd_dict_decompress(const uint8_t* dict, uint32_t dict_bytes, const uint8_t* packed,
                                           uint64_t packed_readable, const uint64_t* offsets, const uint32_t* csizes,
                                           void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                                           int32_t* status, uint32_t nchunks, hipStream_t s) {
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_zstd_dict_decompress_kernel, dim3(nchunks), dim3(64), 0, s, dict, dict_bytes, packed,
                       packed_readable, offsets, csizes, out_ptrs, out_bytes, max_bytes, status);
    return hipGetLastError();
}
