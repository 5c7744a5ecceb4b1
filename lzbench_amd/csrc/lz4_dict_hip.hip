// lzbench_amd/csrc/lz4_dict_hip.hip -- LZ4 ragged batches with a shared dictionary (include/lzbench_hip.h 3d).
//
// Every chunk of a batch is compressed as lz4 1.9.3 compresses it when the dictionary lies directly before it in one
// buffer: a fresh stream, LZ4_loadDict, LZ4_compress_fast_continue in prefix mode (lz4.c:1565-1605 ->
// LZ4_compress_generic with byU32, withPrefix64k, dictSmall below 64 KiB of dictionary, else noDictIssue).  Positions
// are the reference's indices: the chunk starts at index 65536 (kB0), the dictionary ends there, so it starts at
// 65536 - dict_bytes (lz4.c:1491-1504).  The dictionary is one device buffer and the chunks are wherever the caller's
// pointers say: an index below kB0 is read from the dictionary in place, one at or above it from the chunk (Src).
//
// Three kernels:
//   lzh_lz4_dict_table_kernel     once per call, one wave: LZ4_loadDict's table (lz4.c:1509-1512: every third
//                                 position up to dictEnd - 8, a later position replacing an earlier one) into temp
//   lzh_lz4_dict_compress_kernel  one wave per chunk: the table copied into LDS, then the reference's greedy parse
//                                 position by position with wave-uniform state; what a position needs of the chunk
//                                 comes from a 256-byte register window (UWin), the candidate's four bytes are the
//                                 one dependent load of a probe; catch-up, LZ4_count and the copies run over the 64
//                                 lanes.  The block is assembled in the chunk's staging slot (in-kernel emission; the
//                                 slot holds LZ4_compressBound, so limitedOutput never fires).
//   lzh_lz4_dict_decode_kernel    one wave per chunk: LZ4_decompress_safe_usingDict's verdicts and bytes
//                                 (lz4.c:1929-2151 with usingExtDict: an offset may reach dict_bytes before the
//                                 chunk's first byte).  The token walk is wave-uniform; literals and matches are
//                                 copied by the 64 lanes.  A match byte's source is the output position
//                                 op - offset + (k mod offset): always before op, so every byte of a match -- the
//                                 overlapping ones and the ones that follow a start in the dictionary into the
//                                 output -- is read from memory written by an earlier sequence, or from the
//                                 dictionary's end where that position is negative.
// This is not the speculative batch parse of lz4c.h (compress_chunk): that function's candidate window, slow
// paths and input ring address one buffer, and the two-source M side is not built into it yet.  The
// header is included for the hash, the sequence layout and the span copy alone; no kernel of another file changes.
#include "lz4c.h"

namespace lz4d {

constexpr int kB0 = 65536;            // the chunk's first index (LZ4_loadDict: currentOffset = 64 KB)
constexpr int kTab = 4096;            // byU32 table entries (LZ4_HASH_SIZE_U32)
// a length past this ends the decoder's length loops: it is past any output (chunks are up to 4 MiB), the sequence
// fails its output check either way, and the sums stay far from the int range
constexpr int kLenMax = 1 << 28;

// Wave-uniform reads through a register window: lane l holds the dword at descriptor offset base + 4l, a read
// picks its dwords with v_readlane.  A read outside the window reloads it at the read's position.
struct UWin {
    uint32_t w = 0;
    int base = -(1 << 30);
    __device__ __forceinline__ uint64_t u64(const Bytes& B, int pos, int lane) {
        const int X = unii(pos + B.sh);
        if (X < base || X - base > 244) {
            base = X & ~3;
            w = ld_b32(B.r, base + 4 * lane);
        }
        const int i = unii((X - base) >> 2);
        const uint32_t s = 8u * ((uint32_t)X & 3u);
        const uint64_t lo = (uint64_t)rdlane(w, i) | ((uint64_t)rdlane(w, i + 1) << 32);
        const uint64_t hi = rdlane(w, i + 2);
        return s ? (lo >> s) | (hi << (64u - s)) : lo;
    }
    __device__ __forceinline__ uint32_t u8(const Bytes& B, int pos, int lane) { return (uint32_t)u64(B, pos, lane) & 0xffu; }
};

// The two sources of the compressor's M side: index i < kB0 is dictionary byte i - lo (lo = kB0 - dict_bytes), else
// chunk byte i - kB0.  Per-lane indices: two buffer loads under complementary lane masks.
struct Src {
    Bytes dict, in;
    int lo;
    __device__ __forceinline__ uint32_t b(int i) const { return i < kB0 ? dict.b(i - lo) : in.b(i - kB0); }
    // the four bytes at a wave-uniform index
    __device__ __forceinline__ uint32_t u32(int i) const {
        if (i + 4 <= kB0) return uni(dict.w32(i - lo));
        if (i >= kB0) return uni(in.w32(i - kB0));
        return uni(b(i) | (b(i + 1) << 8) | (b(i + 2) << 16) | (b(i + 3) << 24));
    }
};

// LZ4_count(ip, match, limit) with ip = chunk position p (index p + kB0) and match = index m: 64 bytes a step
__device__ __forceinline__ int count_fwd(const Src& S, int p, int m, int limit, int lane) {
    int cnt = 0;
    for (;;) {
        const int k = cnt + lane;
        const bool eq = p + k < limit && S.in.b(p + k) == S.b(m + k);
        const int f = ffs64(ballot(!eq));
        cnt += f;
        if (f < LZH_WAVE) break;
    }
    return cnt;
}

// the catch-up of lz4.c:1019: bytes equal before chunk position p and index m, down to the anchor and to lowLimit
// (index low: the dictionary's first byte)
__device__ __forceinline__ int count_bwd(const Src& S, int p, int m, int anchor, int low, int lane) {
    int bk = 0;
    for (;;) {
        const int k = bk + lane;
        const bool eq = p - 1 - k >= anchor && m - 1 - k >= low && S.in.b(p - 1 - k) == S.b(m - 1 - k);
        const int f = ffs64(ballot(!eq));
        bk += f;
        if (f < LZH_WAVE) break;
    }
    return bk;
}

// one sequence (has_match) or the last literals at op of the staging slot; returns the new op
__device__ __forceinline__ int put_seq(const Bytes& in, const Bytes& out, int op, int anchor, int lit, bool has_match,
                                       int off, int ml, int lane) {
    const lz4v3::SeqLayout L(lit, has_match, ml);
    if (lane == 0) out.st8(op, L.token);
    for (int b = lane; b < L.lx; b += LZH_WAVE) out.st8(op + 1 + b, b == L.lx - 1 ? L.lrem : 255u);
    copy_span(in, anchor, out, op + L.lit0, lit, lane, LZH_WAVE);
    if (has_match) {
        if (lane < 2) out.st8(op + L.lit1 + lane, lane ? ((uint32_t)off >> 8) : ((uint32_t)off & 0xffu));
        for (int b = lane; b < L.mx; b += LZH_WAVE) out.st8(op + L.lit1 + 2 + b, b == L.mx - 1 ? L.mrem : 255u);
    }
    return op + L.total;
}

}  // namespace lz4d

extern "C" __global__ void __launch_bounds__(64)
lzh_lz4_dict_table_kernel(const uint8_t* dict, uint32_t dict_bytes, uint32_t* tab) {
    __shared__ uint32_t t[lz4d::kTab];
    const int lane = threadIdx.x;
    for (int i = lane; i < lz4d::kTab; i += LZH_WAVE) t[i] = 0;
    __syncthreads();
    Bytes d;
    d.init(dict, (uint64_t)dict_bytes + 16);
    // positions 0, 3, 6, .. <= dict_bytes - 8; indices grow with the position, so the last writer of a slot is its
    // largest index (an empty slot and index 0, the first byte of a 64 KiB dictionary, are both 0, as in lz4.c)
    const int npos = ((int)dict_bytes - 8) / 3 + 1;
    for (int j = lane; j < npos; j += LZH_WAVE) {
        const int p = 3 * j;
        const uint64_t v = d.w40(p);
        const uint32_t h = lz4v3::hash_of<false>((uint32_t)v, (uint32_t)(v >> 32));
        atomicMax(&t[h], (uint32_t)(lz4d::kB0 - (int)dict_bytes + p));
    }
    __syncthreads();
    for (int i = lane; i < lz4d::kTab; i += LZH_WAVE) tab[i] = t[i];
}

extern "C" __global__ void __launch_bounds__(64)
lzh_lz4_dict_compress_kernel(const uint8_t* dict, uint32_t dict_bytes, const uint32_t* tab_g, const void* const* in_ptrs,
                             const uint64_t* in_bytes, uint64_t max_bytes, int acc, uint8_t* stage, uint64_t stride,
                             uint32_t* csizes) {
    using namespace lz4d;
    __shared__ __attribute__((aligned(16))) uint32_t tab[kTab];
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint8_t* inp;
    int n;
    if (!ragged_span(in_ptrs, in_bytes, chunk, max_bytes, inp, n)) {
        if (lane == 0) csizes[chunk] = 0;
        return;
    }
    Src S;
    S.in.init(inp, (uint64_t)n + 16);
    S.dict.init(dict, (uint64_t)dict_bytes + 16);
    S.lo = kB0 - (int)dict_bytes;
    const Bytes& in = S.in;
    Bytes out;
    out.init(stage + chunk * stride, stride);
    for (int i = lane; i < kTab; i += LZH_WAVE) tab[i] = tab_g[i];
    __syncthreads();
    volatile LDSA uint32_t* T = (volatile LDSA uint32_t*)tab;

    // dictSmall (lz4.c:1601-1602): a candidate below the dictionary's first index is skipped (empty slots too);
    // noDictIssue with 64 KiB: index 0 is a candidate like any other
    const uint32_t idx_lim = dict_bytes < 65536u ? (uint32_t)S.lo : 0u;
    const int mfl1 = n - lz4v3::kMfLimit + 1;          // mflimitPlusOne
    const int mlimit = n - lz4v3::kLastLiterals;       // matchlimit
    int op = 0, anchor = 0;
    UWin W;

    if (n >= lz4v3::kMinLength) {
        {   // the first position enters the table before the first search (lz4.c:924)
            const uint64_t v = W.u64(in, 0, lane);
            T[lz4v3::hash_of<false>((uint32_t)v, (uint32_t)(v >> 32) & 0xffu)] = (uint32_t)kB0;
        }
        int ip = 1;
        for (;;) {
            int match = 0, lit = 0;
            bool found = false;
            {   // search (lz4.c:956-1014)
                int fwd = ip, step = 1, nb = acc << 6;
                for (;;) {
                    const int cur = fwd;
                    fwd += step;
                    step = nb++ >> 6;
                    if (fwd > mfl1) break;
                    const uint64_t v = W.u64(in, cur, lane);
                    const uint32_t h = lz4v3::hash_of<false>((uint32_t)v, (uint32_t)(v >> 32) & 0xffu);
                    const uint32_t cand = uni(T[h]);
                    T[h] = (uint32_t)(cur + kB0);
                    if (cand < idx_lim) continue;
                    if (cand + 65535u < (uint32_t)(cur + kB0)) continue;
                    if (S.u32((int)cand) == (uint32_t)v) {
                        ip = cur;
                        match = (int)cand;
                        found = true;
                        break;
                    }
                }
            }
            if (!found) break;
            {
                const int bk = count_bwd(S, ip, match, anchor, S.lo, lane);
                ip -= bk;
                match -= bk;
                lit = ip - anchor;
            }
            bool end = false;
            for (;;) {   // _next_match (lz4.c:1048-1196)
                const int off = ip + kB0 - match;
                const int ml = count_fwd(S, ip + lz4v3::kMinMatch, match + lz4v3::kMinMatch, mlimit, lane);
                op = put_seq(in, out, op, anchor, lit, true, off, ml, lane);
                ip += ml + lz4v3::kMinMatch;
                anchor = ip;
                if (ip >= mfl1) { end = true; break; }
                {
                    const uint64_t v2 = W.u64(in, ip - 2, lane);
                    T[lz4v3::hash_of<false>((uint32_t)v2, (uint32_t)(v2 >> 32) & 0xffu)] = (uint32_t)(ip - 2 + kB0);
                }
                const uint64_t v = W.u64(in, ip, lane);
                const uint32_t h = lz4v3::hash_of<false>((uint32_t)v, (uint32_t)(v >> 32) & 0xffu);
                const uint32_t cand = uni(T[h]);
                T[h] = (uint32_t)(ip + kB0);
                if (cand >= idx_lim && cand + 65535u >= (uint32_t)(ip + kB0) && S.u32((int)cand) == (uint32_t)v) {
                    match = (int)cand;
                    lit = 0;
                    continue;
                }
                break;
            }
            if (end) break;
            ip++;
        }
    }
    op = put_seq(in, out, op, anchor, n - anchor, false, 0, 0, lane);
    if (lane == 0) csizes[chunk] = (uint32_t)op;
}

// status[i]: the decoded size, or negative (the walk's -(position in the block) - 1, as lz4.c:2163 counts it)
extern "C" __global__ void __launch_bounds__(64)
lzh_lz4_dict_decode_kernel(const uint8_t* dict, uint32_t dict_bytes, const uint8_t* packed, uint64_t packed_readable,
                           const uint64_t* offsets, const uint32_t* csizes, void* const* out_ptrs,
                           const uint64_t* out_bytes, uint64_t max_bytes, int32_t* status) {
    using namespace lz4d;
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint64_t ob = uni64(out_bytes[chunk]);
    if (ob > max_bytes) {
        if (lane == 0) status[chunk] = -1;
        return;
    }
    const uint64_t soff = uni64(offsets[chunk]);
    const uint32_t cs = uni(csizes[chunk]);
    uint8_t* outp = (uint8_t*)uni64((uint64_t)out_ptrs[chunk]);
    if (soff > packed_readable || (uint64_t)cs > packed_readable - soff) {   // the block is not inside packed
        if (lane == 0) status[chunk] = -1;
        return;
    }
    Bytes in, out, dc;
    in.init_dw(packed + soff, cs);   // (dword reads of the block's last bytes stay in range)
    out.init(outp, ob);
    dc.init(dict, (uint64_t)dict_bytes + 16);
    const int cap = (int)ob, iend = (int)cs, D = (int)dict_bytes;
    int res;
    if ((uint64_t)cs == ob) {                       // stored raw
        copy_span(in, 0, out, 0, cap, lane, LZH_WAVE);
        res = cap;
    } else if (cap == 0) {
        res = (cs == 1 && uni(in.b(0)) == 0) ? 0 : -1;
    } else if (cs == 0 || cs > (1u << 30)) {   // (no block of a chunk of up to 4 MiB is that long)
        res = -1;
    } else {
        UWin W;
        int ip = 0, op = 0;
        int synced = 0;          // output bytes [0, synced) are visible to this wave's loads
        for (;;) {
            if (ip >= iend) { res = -ip - 1; break; }
            const uint32_t tok = W.u8(in, ip++, lane);
            int lit = (int)(tok >> 4);
            if (lit == 15) {   // (lz4.c:1707-1729: an error only with no room at the start)
                if (ip >= iend - 15) { res = -ip - 1; break; }
                uint32_t s;
                do {
                    s = W.u8(in, ip++, lane);
                    lit += (int)s;
                    if (ip >= iend - 15 || lit > kLenMax) break;
                } while (s == 255);
            }
            if (op + lit > cap - lz4v3::kMfLimit || ip + lit > iend - 8) {
                // the last sequence: it consumes the input exactly and fits the output
                if (ip + lit != iend || op + lit > cap) { res = -ip - 1; break; }
                copy_span(in, ip, out, op, lit, lane, LZH_WAVE);
                res = op + lit;
                break;
            }
            copy_span(in, ip, out, op, lit, lane, LZH_WAVE);
            ip += lit;
            op += lit;
            const int off = (int)((uint32_t)W.u64(in, ip, lane) & 0xffffu);
            ip += 2;
            int ml = (int)(tok & 15u);
            if (ml == 15) {
                uint32_t s;
                bool bad = false;
                do {
                    s = W.u8(in, ip++, lane);
                    ml += (int)s;
                    if (ip >= iend - lz4v3::kLastLiterals + 1 || ml > kLenMax) { bad = true; break; }
                } while (s == 255);
                if (bad) { res = -ip - 1; break; }
            }
            ml += lz4v3::kMinMatch;
            if (off > op + D) { res = -ip - 1; break; }                        // before the dictionary's first byte
            if (op + ml > cap - lz4v3::kLastLiterals) { res = -ip - 1; break; }   // the last 5 bytes are literals
            if (off == 0) {   // (the match reads itself: zeros, as the CPU restatement of this project defines it)
                for (int k = lane; k < ml; k += LZH_WAVE) out.st8(op + k, 0);
                op += ml;
                continue;
            }
            // sources in [op - off, op - off + min(ml, off)): whatever of it this wave wrote since the last fence
            // must have landed before the loads
            if (op - off + min(ml, off) > synced) {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                synced = op;
            }
            const bool wraps = off < ml;
            for (int k = lane; k < ml; k += LZH_WAVE) {
                const int p = op - off + (wraps ? k % off : k);
                const uint32_t b = p < 0 ? dc.b(D + p) : out.b(p);
                out.st8(op + k, b);
            }
            op += ml;
        }
    }
    if (lane == 0) status[chunk] = res;
}

#include "launch.h"

hipError_t lzh_launch_lz4_dict(const uint8_t* dict, uint32_t dict_bytes, uint32_t* tab, const LzhBatch& B, int acc,
                               const LzhSlots& S, uint32_t* csizes, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_lz4_dict_table_kernel, dim3(1), dim3(64), 0, s, dict, dict_bytes, tab);
    hipLaunchKernelGGL(lzh_lz4_dict_compress_kernel, dim3(B.nchunks), dim3(64), 0, s, dict, dict_bytes,
                       (const uint32_t*)tab, B.ptrs, B.bytes, B.max_bytes, acc, S.stage, S.stride, csizes);
    return hipGetLastError();
}

hipError_t lzh_launch_lz4_dict_decompress(const uint8_t* dict, uint32_t dict_bytes, const uint8_t* packed,
                                          uint64_t packed_readable, const uint64_t* offsets, const uint32_t* csizes,
                                          void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                                          int32_t* status, uint32_t nchunks, hipStream_t s) {
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_lz4_dict_decode_kernel, dim3(nchunks), dim3(64), 0, s, dict, dict_bytes, packed,
                       packed_readable, offsets, csizes, out_ptrs, out_bytes, max_bytes, status);
    return hipGetLastError();
}
