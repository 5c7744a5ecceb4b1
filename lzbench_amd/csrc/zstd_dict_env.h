// lzbench_amd/csrc/zstd_dict_env.h -- what the zstd dictionary compressors share around their walks: level 1
// (zstd_dict_parse.h, zstd_dict_hip.hip; include/lzbench_hip.h 3f) and level 3 (zstd_dfast_dict_parse.h,
// zstd_dfast_dict_hip.hip; 3h).  The walks, zdd::ext_block and zfd::ext_block, restate two reference functions and stay
// two; each runs over an environment E that supplies the memory side, and the byte side of E, the two-segment count, the
// stepping of the class enumeration and, on the device, the frame of a match kernel around its walk are here, once.
// No kernel is defined here.
//
// The first part is plain C++ (the stand-alone host walks compile it with g++); the second is device code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZDE_HD __host__ __device__
#else
#define ZDE_HD
#endif

namespace zde {

// ZSTD_count_2segments for a match at chunk position a against virtual position m, in a block of n bytes: the match
// side may run from the dictionary's end on into the chunk's start (E.crossed(): it did, by at least one byte)
template <class Env>
ZDE_HD int count2(Env& E, int a, int m, int n) {
    if (m >= 0) return E.count_fwd(a, m, n - a);
    const int room = -m < n - a ? -m : n - a;
    const int c = E.count_fwd(a, m, room);
    if (c != -m) return c;
    const int c2 = E.count_fwd(a + c, 0, n - (a + c));
    if (c2 > 0) E.crossed();
    return c + c2;
}

// The byte side of a plain host environment: two byte arrays (16 readable bytes after each) at virtual positions
// (p >= 0: chunk byte p; p < 0: dictionary byte D + p) and the recorder of the stored sequences.
struct HostBytes {
    const uint8_t* dict;
    uint32_t D;
    const uint8_t* src;
    uint32_t* out;      // (ll, ml, offBase) triples, or null
    uint64_t cap, ns, nl;
    const uint8_t* at(int p) const { return p >= 0 ? src + p : dict + D + p; }
    uint32_t r32(int p) const { const uint8_t* q = at(p); return q[0] | (q[1] << 8) | (q[2] << 16) | ((uint32_t)q[3] << 24); }
    uint64_t r64(int p) const { return (uint64_t)r32(p) | ((uint64_t)r32(p + 4) << 32); }
    int count_fwd(int a, int b, int maxn) const {
        int c = 0;
        while (c < maxn && src[a + c] == *at(b + c)) c++;
        return c;
    }
    int count_bwd(int a, int b, int maxn) const {
        int c = 0;
        while (c < maxn && src[a - 1 - c] == *at(b - 1 - c)) c++;
        return c;
    }
    void crossed() const {}
    void seq(int, int ll, uint32_t offBase, uint32_t ml) {
        if (out && ns < cap) { out[3 * ns] = (uint32_t)ll; out[3 * ns + 1] = ml; out[3 * ns + 2] = offBase; }
        ns++;
        nl += (uint64_t)ll;
    }
};

// The class enumerations (zdd::classes_for, zfd::classes_for) visit one chunk size per set of parameters: these change
// only where n + D passes a power of two (srcLog; the three table bounds are powers of two), so after n comes the n
// whose n + D is the next power of two plus one, and max_chunk at the latest.
ZDE_HD inline uint64_t next_class_n(uint64_t n, uint64_t D, uint64_t max_chunk) {
    uint64_t t = 64;
    while (t < n + D) t <<= 1;
    const uint64_t next = t + 1 - D;
    return next > n && next <= max_chunk ? next : max_chunk;
}

// ceil log2 of a batch's largest dictionary + chunk, 6 at the least (ZSTD_HASHLOG_MIN): what caps the table logs of any
// frame of the batch
ZDE_HD inline uint32_t total_log(uint64_t dict_bytes, uint64_t max_bytes) {
    const uint64_t t = dict_bytes + (max_bytes ? max_bytes : 1);
    uint32_t lg = 6;
    while ((1ull << lg) < t) lg++;
    return lg;
}

// a kernel's class argument from the host's enumeration (a level's own further arrays are its launcher's to copy)
template <class Arg, class Classes>
inline void fill_class_arg(Arg& C, const Classes& K) {
    C.count = K.count;
    for (uint32_t i = 0; i < K.count; i++) { C.hlog[i] = K.hlog[i]; C.mls[i] = K.mls[i]; C.off[i] = K.off[i]; }
}

}  // namespace zde

#ifdef __HIPCC__
// ------------------------------------------------------------------------- device side: one wave per chunk
#include "zstdc.h"
#include "launch.h"

namespace zde {

// equal bytes at x[a..] and y[b..], at most maxn; wave-parallel, 256 bytes a round (zc::count_fwd over two views)
__device__ int count_fwd2(const Bytes& x, int a, const Bytes& y, int b, int maxn, int lane) {
    int n = 0;
    while (n < maxn) {
        const int off = n + 4 * lane;
        uint32_t first = 64 * 4;
        if (off < maxn) {
            const uint32_t v = ld_u32(x.r, a + off + x.sh) ^ ld_u32(y.r, b + off + y.sh);
            int eq = v ? (int)(__builtin_ctz(v) >> 3) : 4;
            if (off + eq > maxn) eq = maxn - off;
            if (eq < 4) first = (uint32_t)(4 * lane + eq);
        }
        const uint64_t m = ballot(first < 256u);
        if (m) return n + (int)rdlane(first, ffs64(m));
        n += 256;
    }
    return maxn;
}

// bytes equal going backwards from x[a - 1] / y[b - 1], at most maxn
__device__ int count_bwd2(const Bytes& x, int a, const Bytes& y, int b, int maxn, int lane) {
    int n = 0;
    while (n < maxn) {
        const int k = n + lane;
        const bool stop = k >= maxn || x.b(a - 1 - k) != y.b(b - 1 - k);
        const uint64_t m = ballot(stop);
        if (m) return n + ffs64(m);
        n += 64;
    }
    return maxn;
}

// The byte side of a walk's environment on one wave: uniform loads of the chunk and of the dictionary, counts over the
// 64 lanes, sequences and literals into the frame's store.  A level's WaveEnv adds its tables and its r64.
struct WaveBytes {
    const Bytes& in;
    const Bytes& dict;
    int D;
    zc::SeqOut& O;
    int lane;
    __device__ __forceinline__ uint32_t r32(int p) const { return p >= 0 ? uni(in.w32(p)) : uni(dict.w32(max(D + p, 0))); }
    __device__ __forceinline__ int count_fwd(int a, int b, int maxn) const {
        return b >= 0 ? count_fwd2(in, a, in, b, maxn, lane) : count_fwd2(in, a, dict, D + b, maxn, lane);
    }
    __device__ __forceinline__ int count_bwd(int a, int b, int maxn) const {
        return b >= 0 ? count_bwd2(in, a, in, b, maxn, lane) : count_bwd2(in, a, dict, D + b, maxn, lane);
    }
    __device__ __forceinline__ void crossed() const {}
    __device__ __forceinline__ void seq(int from, int ll, uint32_t offBase, uint32_t mlen) const {
        zc::lit_copy(in, from, O.lits, O.nl, ll, lane);
        O.nl += ll;
        O.put(lane, (uint32_t)ll, offBase, mlen);
    }
};

// A match kernel around its walk.  The frame's scratch starts with the header the ragged entropy kernels read: the
// counts of sequences and of literal bytes, the two repcodes, and at 32 whether the frame is stored raw.  The three
// steps are separate functions and the kernels keep the test in front of the first and their two views of the input
// (an open step that returns false, or one struct for views and store, moved the match kernels' code:
// profiles/zstd_dict_shared/README.md).
//
// open, for a chunk that gets no parse (below 7 bytes, or no table for it): the header of a frame stored raw
__device__ __forceinline__ void raw_header(rsrc_t hdr, int lane) {
    if (lane == 0) { st_b32(hdr, 32, 1u); st_b32(hdr, 0, 0u); st_b32(hdr, 4, 0u); }
}

// the empty sequence store of a block of bsize bytes in the frame's scratch fs
__device__ __forceinline__ void seq_store(zc::SeqOut& O, uint8_t* fs, uint64_t seq_off, uint64_t lit_off, uint32_t bsize) {
    O.seq = make_rsrc(fs + seq_off, (uint32_t)(lit_off - seq_off));
    O.lits.init(fs + lit_off, bsize + 64);
    O.ns = 0;
    O.nl = 0;
}

// close: the literals after the last sequence, [anchor, sn), then the header
__device__ __forceinline__ void close_frame(rsrc_t hdr, const Bytes& in, zc::SeqOut& O, int anchor, int sn,
                                            const uint32_t rep[2], int lane) {
    copy_span(in, anchor, O.lits, O.nl, sn - anchor, lane, LZH_WAVE);   // last literals
    O.nl += sn - anchor;
    if (lane == 0) {
        st_b32(hdr, 0, (uint32_t)O.ns);
        st_b32(hdr, 4, (uint32_t)O.nl);
        st_b32(hdr, 8, rep[0]);
        st_b32(hdr, 12, rep[1]);
        st_b32(hdr, 32, 0u);
    }
}

// The launch chain of a compress call, every launch on s (a captured call is a chain of kernel nodes): the table region
// zeroed, the dictionary's fill of every class (none for a dictionary too short to index), one wave per chunk.
template <class ZeroK, class TableK, class MatchK, class Arg>
inline hipError_t launch_chain(ZeroK zero, TableK table, MatchK match, const Arg& C, uint32_t tables_bytes, uint32_t nfill,
                               const uint8_t* dict, uint32_t dict_bytes, uint8_t* tables, const LzhBatch& B, int level,
                               const LzhSlots& S, const zc::Layout& Lo, uint32_t tab_cap, hipStream_t s) {
    hipLaunchKernelGGL(zero, dim3((tables_bytes / 4 + 255) / 256), dim3(256), 0, s, (uint32_t*)tables, tables_bytes / 4);
    if (nfill)
        hipLaunchKernelGGL(table, dim3((nfill + 255) / 256, C.count), dim3(256), 0, s, dict, dict_bytes, nfill,
                           (uint32_t*)tables, C);
    hipLaunchKernelGGL(match, dim3(B.nchunks), dim3(64), 0, s, dict, dict_bytes, (const uint8_t*)tables, C, B.ptrs,
                       B.bytes, B.max_bytes, level, S.recs, S.rec_stride, Lo.seq_off, Lo.lit_off, Lo.tab_off, tab_cap);
    return hipGetLastError();
}

}  // namespace zde
#endif  // __HIPCC__
