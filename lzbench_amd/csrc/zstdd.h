// lzbench_amd/csrc/zstdd.h -- the one-wave-per-frame zstd decoder's device code (namespace zstdd).  The kernels are
// in the units that include it, each with its own flags: decode_hip.hip, zstd_ragged_decode_hip.hip, zstd_dict_hip.hip.
#pragma once
#include "decode_win.h"
// zstd frames (RFC 8878), the decode side of lzbench's zstd rows (compressors.cpp:1767-1773:
// ZSTD_decompressDCtx of one frame per chunk).  Reference decoder: zstd 1.5.2
//   frame / blocks       zstd/lib/decompress/zstd_decompress.c (ZSTD_decompressFrame)
//   literals, sequences  zstd/lib/decompress/zstd_decompress_block.c (ZSTD_decodeLiteralsBlock,
//                        ZSTD_decodeSeqHeaders, ZSTD_buildFSETable, ZSTD_decodeSequence,
//                        ZSTD_decompressSequences_body)
//   Huffman              zstd/lib/decompress/huf_decompress.c (HUF_readDTableX1, 1X1 / 4X1 streams;
//                        the 1X2 / 4X2 acceptance rules where HUF_selectDecoder picks X2)
//   FSE headers          zstd/lib/common/entropy_common.c (FSE_readNCount, HUF_readStats),
//                        zstd/lib/common/fse_decompress.c (weights: two interleaved states)
// One wave per frame.  Entropy decoding is inherently sequential, so it runs as wave-uniform
// scalar code (every lane holds the same state; tables in LDS read at uniform addresses); the
// backward bitstreams are read through 512-byte register windows (v_readlane, no memory round
// trip per refill).  Literals are decoded into the tail of the chunk's own output region (the
// frame content size is known), and the sequences are executed with the LZ4 decoder's group
// emitter: up to 64 sequences per group, one output byte per lane per pass, through the LDS
// output window.
// Scope: frames as lzbench writes them (content size present, no dictionary), with or without the
// XXH64 content checksum (verified);
// others return kErrUnsupported.  Valid frames decode to the reference's bytes; corrupt frames
// are rejected without faulting, with the reference's accept / reject verdict (tests/test_gpu_zstd.py).
namespace zstdd {

constexpr int kZW = 2048;               // LDS output window (zstd offsets are mostly far anyway)
typedef owin::SinkT<kZW> ZSink;
constexpr int kErrCorrupt = -1, kErrUnsupported = -2, kErrChecksum = -1;

// XXH64 (seed 0) of out[0, len) -- /root/reference/zstd/lib/common/xxhash.h XXH64_endian_align --
// by the whole wave: lane j loads 32-byte stripe j of each 2 KiB batch (L1-bypassing: the bytes
// were just stored by this wave), the four accumulators take the stripes in order (wave-uniform)
__device__ __forceinline__ uint64_t xxh_rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t xxh64_round(uint64_t acc, uint64_t in) {
    return xxh_rotl64(acc + in * 0xC2B2AE3D27D4EB4FULL, 31) * 0x9E3779B185EBCA87ULL;
}
__device__ uint64_t xxh64_wave(const Bytes& b, int len, int lane) {
    constexpr uint64_t P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL,
                       P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
    auto rd32 = [&](int q) -> uint32_t {
        return b.b_sc1(q) | (b.b_sc1(q + 1) << 8) | (b.b_sc1(q + 2) << 16) | (b.b_sc1(q + 3) << 24);
    };
    uint64_t h;
    int p = 0;
    if (len >= 32) {
        uint64_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0ull - P1;
        const int ns = len / 32;
        for (int s0 = 0; s0 < ns; s0 += 64) {
            const int q = (s0 + lane) * 32;
            const bool in = s0 + lane < ns;
            uint32_t w[8];
#pragma unroll
            for (int k = 0; k < 8; k++) w[k] = in ? rd32(q + 4 * k) : 0u;
            const int m = min(64, ns - s0);
            for (int j = 0; j < m; j++) {
                v1 = xxh64_round(v1, (uint64_t)rdlane(w[1], j) << 32 | rdlane(w[0], j));
                v2 = xxh64_round(v2, (uint64_t)rdlane(w[3], j) << 32 | rdlane(w[2], j));
                v3 = xxh64_round(v3, (uint64_t)rdlane(w[5], j) << 32 | rdlane(w[4], j));
                v4 = xxh64_round(v4, (uint64_t)rdlane(w[7], j) << 32 | rdlane(w[6], j));
            }
        }
        p = ns * 32;
        h = xxh_rotl64(v1, 1) + xxh_rotl64(v2, 7) + xxh_rotl64(v3, 12) + xxh_rotl64(v4, 18);
        h = (h ^ xxh64_round(0, v1)) * P1 + P4;
        h = (h ^ xxh64_round(0, v2)) * P1 + P4;
        h = (h ^ xxh64_round(0, v3)) * P1 + P4;
        h = (h ^ xxh64_round(0, v4)) * P1 + P4;
    } else {
        h = P5;
    }
    h += (uint64_t)len;
    for (; p + 8 <= len; p += 8) {
        const uint64_t k = (uint64_t)uni(rd32(p + 4)) << 32 | uni(rd32(p));
        h = xxh_rotl64(h ^ xxh64_round(0, k), 27) * P1 + P4;
    }
    if (p + 4 <= len) {
        h = xxh_rotl64(h ^ ((uint64_t)uni(rd32(p)) * P1), 23) * P2 + P3;
        p += 4;
    }
    for (; p < len; p++) h = xxh_rotl64(h ^ ((uint64_t)uni(b.b_sc1(p)) * P5), 11) * P1;
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}
#ifndef LZH_ZSTD_DEBUG
#define LZH_ZSTD_DEBUG 0
#endif
// corrupt: -1, or (debug builds) -(10000 + source line) to locate the failing check
#define ZC (LZH_ZSTD_DEBUG ? -(10000 + __LINE__) : kErrCorrupt)
// phase clocks (debug builds with -DLZH_ZSTD_STATS=1; the launcher prints them)
#ifndef LZH_ZSTD_STATS
#define LZH_ZSTD_STATS 0
#endif
constexpr int kZClk = 8;
#define ZCLK(F, i) do { if (LZH_ZSTD_STATS) { const uint64_t t_ = __builtin_amdgcn_s_memtime(); (F).clk[i] += t_ - (F).clk_last; (F).clk_last = t_; } } while (0)
constexpr int kBlockMax = 128 * 1024;
constexpr int kHufLogMax = 12;          // HUF_TABLELOG_MAX (huf.h:119): the decoder accepts 12

// literal-length / match-length codes: baseline and extra bits (RFC 8878 3.1.1.3.2.1.1;
// common/zstd_internal.h LL_bits / ML_bits) and the predefined distributions (3.1.1.3.2.2;
// LL/ML/OF_defaultNorm)
LZH_HDR_VAR __constant__ uint32_t kLLBase[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10,   11,   12,   13,    14,    15,    16,   18,
                                     20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
LZH_HDR_VAR __constant__ uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,  0,  0,  0,  1,  1,
                                    1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
LZH_HDR_VAR __constant__ uint32_t kMLBase[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14,  15,  16,  17,  18,   19,   20,
                                     21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,  33,  34,  35,  37,   39,   41,
                                     43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
LZH_HDR_VAR __constant__ uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                    0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
LZH_HDR_VAR __constant__ int8_t kLLNorm[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                   2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
LZH_HDR_VAR __constant__ int8_t kMLNorm[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,
                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
LZH_HDR_VAR __constant__ int8_t kOFNorm[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};

// FSE decoding-table cell, 32 bits: next-state base (9) | nbBits << 9 (4) | extra bits << 13 (5)
// | symbol << 18 (6).  For LL/ML the symbol is the length code (its baseline comes from a constant
// table off the state chain), for OF the offset code (= its extra-bit count).
typedef uint32_t Cell;
__device__ __forceinline__ uint32_t c_next(Cell c) { return c & 511u; }
__device__ __forceinline__ int c_nb(Cell c) { return (int)((c >> 9) & 15u); }
__device__ __forceinline__ int c_add(Cell c) { return (int)((c >> 13) & 31u); }
__device__ __forceinline__ uint32_t c_sym(Cell c) { return c >> 18; }

// per-wave LDS
struct Lds {
    uint16_t huf[1 << kHufLogMax];      // Huffman decoding table: symbol | nbBits << 8
    Cell ll[512], ml[512], of[256];     // sequence FSE tables (ZSTD_seqSymbol's fields, packed)
    Cell wt[64];                       // FSE table of the Huffman weights (accuracy <= 6)
    uint8_t weights[256];
    int16_t norm[256];
    uint16_t next[256];
    // (the split decoder's header kernel allocates the fields above only)
    uint32_t base[36 + 53];             // literal-length / match-length baselines (kLLBase, kMLBase)
    uint8_t win[kZW + 3 * LZH_WAVE];     // output window | start marks + scratch (groups::emit_group)
};
constexpr size_t kLdsHdr = offsetof(Lds, base);

__device__ __forceinline__ uint32_t lds_u32(const LDSA uint32_t* p) { return uni(*(volatile const LDSA uint32_t*)p); }
__device__ __forceinline__ uint32_t lds_u16(const LDSA uint16_t* p) { return uni(*(volatile const LDSA uint16_t*)p); }
__device__ __forceinline__ uint32_t lds_u8(const LDSA uint8_t* p) { return uni(*(volatile const LDSA uint8_t*)p); }
__device__ __forceinline__ Cell lds_cell(const LDSA Cell* p) { return uni(*(volatile const LDSA uint32_t*)p); }
__device__ __forceinline__ int hb32(uint32_t v) { return 31 - __builtin_clz(v); }   // v > 0

// uniform little-endian reads from a forward register window (Win) over the frame
__device__ __forceinline__ uint32_t fbyte(ZWin& w, int pos, int lane) { w.ensure(pos, lane); return uni(w.byte(pos)); }
__device__ __forceinline__ uint32_t fword(ZWin& w, int pos, int lane) {   // bytes pos..pos+3
    w.ensure(pos, lane);
    const int x = pos + w.sh, d = (x - w.wb) >> 2;
    const uint32_t a = d < 64 ? rdlane(w.w0, d) : rdlane(w.w1, d - 64);
    const uint32_t b = d + 1 < 64 ? rdlane(w.w0, d + 1) : rdlane(w.w1, d + 1 - 64);
    return uni(__builtin_amdgcn_alignbyte(b, a, (uint32_t)x & 3u));
}

// Backward bitstream (RFC 8878 4.1 / bitstream.h BIT_DStream), wave-uniform.  Positions are
// bit indices in the descriptor's byte space: the stream is bits [lo, P) still unread, the next
// n-bit field is bits [P - n, P) (most significant first).  c holds the 64 bits from the
// dword-aligned bit D8 (P - D8 in [32, 63] after a reload, so any field of <= 32 bits is in
// c); source dwords come from a 512-byte register window (v_readlane) that slides down.
struct BackBits {
    rsrc_t r;
    int wb;              // descriptor offset of the window start (multiple of 4)
    uint32_t w0, w1;     // window dwords [wb, wb + 256), [wb + 256, wb + 512)
    int lo, P, D8;
    uint64_t c;

    __device__ __forceinline__ uint32_t dw(int D) const {
        const int d = (D - wb) >> 2;
        return rdlane(d < 64 ? w0 : w1, d & 63);
    }
    __device__ __forceinline__ void cover(int D0, int D1, int lane) {   // bytes [D0, D1), D1 - D0 <= 256
        if (D0 >= wb && D1 <= wb + 512) return;
        if (D0 >= wb - 256 && D1 <= wb + 256) {
            w1 = w0;
            wb -= 256;
            w0 = ld_b32(r, wb + 4 * lane);
            return;
        }
        wb = D1 - 512;
        w0 = ld_b32(r, wb + 4 * lane);
        w1 = ld_b32(r, wb + 256 + 4 * lane);
    }
    __device__ __forceinline__ void reload(int lane) {
        D8 = ((P - 32) >> 5) << 5;
        const int D = D8 >> 3;
        cover(D, D + 8, lane);
        c = ((uint64_t)dw(D + 4) << 32) | dw(D);
    }
    // stream = descriptor bytes [start, start + size) (start including the descriptor shift);
    // false if empty or the end mark is missing
    __device__ __forceinline__ bool init(const Bytes& src, int start, int size, int lane) {
        r = src.r;
        const int s0 = start + src.sh;
        wb = ((s0 + size + 3) & ~3) - 512;
        w0 = ld_b32(r, wb + 4 * lane);
        w1 = ld_b32(r, wb + 256 + 4 * lane);
        lo = 8 * s0;
        if (size <= 0) return false;
        const int X = s0 + size - 1;
        const uint32_t last = (dw(X & ~3) >> (8 * (X & 3))) & 0xffu;
        if (last == 0) return false;
        P = 8 * X + hb32(last);
        reload(lane);
        return true;
    }
    __device__ __forceinline__ int left() const { return P - lo; }
    // next n bits (0 <= n <= 32), consumed; bits below the stream start read as garbage
    // (callers reject a stream that overruns)
    __device__ __forceinline__ uint32_t get(int n, int lane) {
        if (P - n < D8) reload(lane);
        const uint32_t v = (uint32_t)((c >> (P - n - D8)) & ((1ull << n) - 1ull));
        P -= n;
        return v;
    }
    // next n bits (1 <= n <= 32) without consuming them, zero-padded below the stream start
    __device__ __forceinline__ uint32_t peek(int n, int lane) {
        if (P - n < D8) reload(lane);
        uint32_t v = (uint32_t)((c >> (P - n - D8)) & ((1ull << n) - 1ull));
        if (P - n < lo) v &= (uint32_t)(~0ull << (lo - (P - n)));
        return v;
    }
    __device__ __forceinline__ void skip(int n) { P -= n; }
};

// value in a VGPR as far as the compiler knows (keeps wave-uniform chains out of the SGPR budget)
__device__ __forceinline__ int vgpr(int x) {
    int y;
    asm volatile("v_mov_b32 %0, %1" : "=v"(y) : "v"(x));
    return y;
}

// The sequences' backward bit stream with its state in vector registers (BackBits' container
// semantics): every read takes n <= 32 bits after making sure P - n >= D8, so a refill always
// moves the 64-bit container down by exactly one dword; the next eight dwords below are kept
// prefetched (bank a in use, bank b in flight).
struct SeqBits {
    rsrc_t r;
    int P, D8, lo, na, nxt;
    uint64_t c;
    uint32_t a0, a1, a2, a3, b0, b1, b2, b3;
    __device__ __forceinline__ bool init(const Bytes& src, int start, int size) {
        r = src.r;
        const int x0 = vgpr(start + src.sh);
        if (size <= 0) return false;
        const int X = x0 + size - 1;
        const uint32_t last = ld_u8(r, X);
        if (last == 0) return false;
        lo = 8 * x0;
        P = 8 * X + hb32(last);
        D8 = ((P - 32) >> 5) << 5;
        const int D = D8 >> 3;
        c = ((uint64_t)ld_b32(r, D + 4) << 32) | ld_b32(r, D);
        a0 = ld_b32(r, D - 4); a1 = ld_b32(r, D - 8); a2 = ld_b32(r, D - 12); a3 = ld_b32(r, D - 16);
        b0 = ld_b32(r, D - 20); b1 = ld_b32(r, D - 24); b2 = ld_b32(r, D - 28); b3 = ld_b32(r, D - 32);
        na = 4;
        nxt = D - 36;
        return true;
    }
    __device__ __forceinline__ int left() const { return P - lo; }
    __device__ __forceinline__ uint32_t get(int n) {
        if (P - n < D8) {
            c = (c << 32) | a0;
            a0 = a1; a1 = a2; a2 = a3;
            D8 -= 32;
            if (--na == 0) {
                a0 = b0; a1 = b1; a2 = b2; a3 = b3;
                b0 = ld_b32(r, nxt); b1 = ld_b32(r, nxt - 4); b2 = ld_b32(r, nxt - 8); b3 = ld_b32(r, nxt - 12);
                nxt -= 16;
                na = 4;
            }
        }
        const uint32_t v = (uint32_t)((c >> (P - n - D8)) & ((1ull << n) - 1ull));
        P -= n;
        return v;
    }
};

// FSE_readNCount (entropy_common.c:70-215) over the frame from byte pos: normalized counts
// into L.norm[0..maxSym], returns the header size in bytes (<= 0: corrupt); *al = accuracy log
__device__ __forceinline__ int read_ncount(ZWin& fw, int pos, int end, int maxSym, int maxLog, LDSA Lds& L, int& al, int& nsym,
                           int lane) {
    for (int i = lane; i < 256; i += LZH_WAVE) L.norm[i] = 0;
    int bit = 0;                                      // bits consumed from pos
    auto peek32 = [&](void) -> uint32_t {
        const int p = pos + (bit >> 3);
        const uint64_t v = ((uint64_t)fword(fw, p + 4, lane) << 32) | fword(fw, p, lane);
        return (uint32_t)(v >> (bit & 7));
    };
    uint32_t bs = peek32();
    int nb = (int)(bs & 15u) + 5;
    if (nb > maxLog) return ZC;
    al = nb;
    bit = 4;
    int remaining = (1 << nb) + 1, threshold = 1 << nb;
    nb++;
    int sym = 0;
    bool prev0 = false;
    for (int guard = 0; guard < 512; guard++) {
        if (prev0) {                                  // 2-bit repeat flags: 3 = three more zeros, go on
            for (int g2 = 0; g2 < 256; g2++) {
                const uint32_t r2 = peek32() & 3u;
                bit += 2;
                sym += (int)r2;
                if (r2 != 3) break;
            }
            if (sym > maxSym) return ZC;
        }
        bs = peek32();
        const int mx = (2 * threshold - 1) - remaining;
        int count;
        if ((int)(bs & (uint32_t)(threshold - 1)) < mx) {
            count = (int)(bs & (uint32_t)(threshold - 1));
            bit += nb - 1;
        } else {
            count = (int)(bs & (uint32_t)(2 * threshold - 1));
            if (count >= threshold) count -= mx;
            bit += nb;
        }
        count--;
        remaining -= count < 0 ? -count : count;
        if (sym > maxSym) return ZC;
        if (lane == 0) L.norm[sym] = (int16_t)count;
        sym++;
        prev0 = count == 0;
        if (remaining < threshold) {
            if (remaining <= 1) break;
            nb = hb32((uint32_t)remaining) + 1;
            threshold = 1 << (nb - 1);
        }
        if (sym > maxSym) break;
    }
    wave_lds_fence();
    if (remaining != 1 || bit > 8 * (end - pos)) return ZC;
    nsym = sym;
    return (bit + 7) >> 3;
}

// FSE_buildDTable (fse_decompress.c:72-160; ZSTD_buildFSETable for the sequence tables):
// symbols spread over the table, then each cell's next-state base and bit count.  Cells are
// (symbol, next-state base | nbBits << 16).
__device__ __forceinline__ void build_fse(LDSA Cell* T, int al, int nsym, LDSA Lds& L, int lane) {
    const int size = 1 << al, mask = size - 1;
    int high = size - 1;
    for (int s = 0; s < nsym; s++) {                  // low-probability symbols at the top
        const int n = (int16_t)lds_u16((const LDSA uint16_t*)&L.norm[s]);
        if (n == -1) {
            if (lane == 0) T[high] = (uint32_t)s << 18;
            high--;
        }
        if (lane == 0) L.next[s] = (uint16_t)(n == -1 ? 1 : n);
    }
    wave_lds_fence();
    const int step = (size >> 1) + (size >> 3) + 3;
    int p = 0;
    for (int s = 0; s < nsym; s++) {
        const int n = (int16_t)lds_u16((const LDSA uint16_t*)&L.norm[s]);
        for (int i = 0; i < n; i++) {
            if (lane == 0) T[p] = (uint32_t)s << 18;
            p = (p + step) & mask;
            while (p > high) p = (p + step) & mask;
        }
    }
    wave_lds_fence();
    for (int u = 0; u < size; u++) {
        const uint32_t s = uni(((volatile const LDSA uint32_t*)T)[u]) >> 18;
        const uint32_t nx = lds_u16(&L.next[s]);
        if (lane == 0) L.next[s] = (uint16_t)(nx + 1);
        const int nb = al - hb32(nx);
        const uint32_t base = (nx << nb) - (uint32_t)size;
        if (lane == 0) T[u] = (s << 18) | ((uint32_t)nb << 9) | base;
        wave_lds_fence();
    }
}

// FSE_buildDTable for the sequence tables (nsym <= 53, size <= 512), lane-parallel, the same cells as
// build_fse: (1) per symbol (lanes): the low-probability symbols' top cells and the running sum C of
// the other counts; (2) per spread step i (lanes, 64 at a time): position (i * step) & mask, kept when
// <= high, its rank among the kept ones gives the symbol (the last s with C[s] <= rank: a binary
// search); (3) per position u ascending (lanes, 64 at a time): the symbol's next-state counter value
// at u -- its initial count plus the same-symbol cells before u -- with the counters in one VGPR
// (lane s holds symbol s's) and the cells of a 64-position batch taken one distinct symbol at a time.
__device__ __forceinline__ void build_fse_par(LDSA Cell* T, int al, int nsym, LDSA Lds& L, int lane) {
    const int size = 1 << al, mask = size - 1;
    const int step = (size >> 1) + (size >> 3) + 3;
    const uint64_t below = (1ull << lane) - 1ull;
    // (1) symbols: lane s (nsym <= 64)
    const int n = lane < nsym ? (int)L.norm[lane] : 0;
    const bool lowp = n == -1;
    const uint64_t lm = ballot(lowp);
    const int nlow = __builtin_popcountll(lm);
    const int high = size - 1 - nlow;
    if (lowp) T[size - 1 - __builtin_popcountll(lm & below)] = (uint32_t)lane << 18;
    int C = n > 0 ? n : 0;                            // exclusive prefix sum of the positive counts
    {
        int x = C;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const int y = __shfl_up(x, k);
            if (lane >= k) x += y;
        }
        C = x - C;
    }
    L.next[lane < 256 ? lane : 0] = lane < nsym ? (uint16_t)C : (uint16_t)0xffffu;
    wave_lds_fence();
    // (2) the spread
    int kept = 0;
    for (int c = 0; c < size; c += LZH_WAVE) {
        const int i = c + lane;
        const int pos = (int)(((uint32_t)i * (uint32_t)step) & (uint32_t)mask);
        const bool valid = i < size && pos <= high;
        const uint64_t vm = ballot(valid);
        const int rank = kept + __builtin_popcountll(vm & below);
        kept += __builtin_popcountll(vm);
        // the last symbol s < nsym with C[s] <= rank
        int lo = 0, hi = nsym - 1;
        while (ballot(valid && lo < hi)) {
            const int mid = (lo + hi + 1) >> 1;
            const bool le = (int)L.next[mid] <= rank;
            if (valid && lo < hi) { lo = le ? mid : lo; hi = le ? hi : mid - 1; }
        }
        if (valid) T[pos] = (uint32_t)lo << 18;
    }
    wave_lds_fence();
    // (3) next states, positions ascending
    int cnt = lowp ? 1 : n;                           // lane s: symbol s's counter
    for (int c = 0; c < size; c += LZH_WAVE) {
        const int u = c + lane;
        const bool on = u < size;
        const uint32_t sym = on ? (T[u] >> 18) : 0xffu;
        int nx = 0;
        for (uint64_t rem = ballot(on); rem;) {
            const int s0 = (int)rdlane(sym, __builtin_ctzll(rem));
            const uint64_t m = ballot(on && sym == (uint32_t)s0) & rem;
            const int base = rdlanei(cnt, s0);
            if (lane_on(m)) nx = base + __builtin_popcountll(m & below);
            if (lane == s0) cnt += __builtin_popcountll(m);
            rem &= ~m;
        }
        if (on) {
            const int nb = al - hb32((uint32_t)nx);
            const uint32_t base = ((uint32_t)nx << nb) - (uint32_t)size;
            T[u] = (sym << 18) | ((uint32_t)nb << 9) | base;
        }
    }
    wave_lds_fence();
}

// sequence-table cells: symbol -> baseline value and extra-bit count (RFC 8878 3.1.1.3.2.1.1)
__device__ __forceinline__ void seq_cells(LDSA Cell* T, int size, int which, int lane) {
    for (int u = lane; u < size; u += LZH_WAVE) {
        const uint32_t c = T[u], s = c >> 18;
        const uint32_t add = which == 0 ? kLLBits[s] : (which == 2 ? kMLBits[s] : s);
        T[u] = c | (add << 13);
    }
    wave_lds_fence();
}

// sequence table for one of LL / OF / ML (ZSTD_buildSeqTable, zstd_decompress_block.c:~560):
// mode 0 predefined, 1 RLE, 2 FSE-compressed, 3 repeat.  Returns bytes consumed, < 0 corrupt.
__device__ __forceinline__ int seq_table(ZWin& fw, int pos, int end, int mode, int which, LDSA Cell* T, int& al, bool& valid,
                         LDSA Lds& L, int lane) {
    const int maxSym = which == 0 ? 35 : (which == 1 ? 31 : 52);
    const int maxLog = which == 1 ? 8 : 9;
    if (mode == 0) {
        const int n = which == 0 ? 36 : (which == 1 ? 29 : 53);
        for (int s = lane; s < n; s += LZH_WAVE)
            L.norm[s] = which == 0 ? kLLNorm[s] : (which == 1 ? kOFNorm[s] : kMLNorm[s]);
        wave_lds_fence();
        al = which == 1 ? 5 : 6;
        build_fse_par(T, al, n, L, lane);
        seq_cells(T, 1 << al, which, lane);
        valid = true;
        return 0;
    }
    if (mode == 1) {
        if (pos >= end) return ZC;
        const int s = (int)fbyte(fw, pos, lane);
        if (s > maxSym) return ZC;
        if (lane == 0) T[0] = (uint32_t)s << 18;
        wave_lds_fence();
        seq_cells(T, 1, which, lane);
        al = 0;
        valid = true;
        return 1;
    }
    if (mode == 2) {
        int nsym = 0;
        const int h = read_ncount(fw, pos, end, maxSym, maxLog, L, al, nsym, lane);
        if (h <= 0) return h < 0 ? h : ZC;
        if (pos + h > end) return ZC;
        build_fse_par(T, al, nsym, L, lane);
        seq_cells(T, 1 << al, which, lane);
        valid = true;
        return h;
    }
    return valid ? 0 : -1;                             // repeat: the previous block's table
}

// Huffman tree description (HUF_readStats, entropy_common.c:271-334; HUF_readDTableX1,
// huf_decompress.c:342-470) at pos.  Returns bytes consumed (< 0 corrupt), *tl = table log.
__device__ __forceinline__ int read_huf(ZWin& fw, const Bytes& src, int pos, int end, LDSA Lds& L, int& tl, int lane) {
    if (pos >= end) return ZC;
    const int hb = (int)fbyte(fw, pos, lane);
    int n, used;
    if (hb >= 128) {                                   // direct 4-bit weights
        n = hb - 127;
        used = 1 + (n + 1) / 2;
        if (pos + used > end) return ZC;
        for (int i = 0; i < n; i++) {
            const uint32_t b = fbyte(fw, pos + 1 + i / 2, lane);
            if (lane == 0) L.weights[i] = (uint8_t)((i & 1) ? (b & 15u) : (b >> 4));
        }
    } else {                                           // FSE-compressed weights, accuracy <= 6
        used = 1 + hb;
        if (pos + used > end || hb == 0) return ZC;
        int al = 0, nsym = 0;
        const int h = read_ncount(fw, pos + 1, pos + 1 + hb, 255, 6, L, al, nsym, lane);
        if (h < 0) return h;
        if (h == 0 || h >= hb) return ZC;
        build_fse(L.wt, al, nsym, L, lane);
        BackBits bb;
        if (!bb.init(src, pos + 1 + h, hb - h, lane)) return ZC;
        // two interleaved states (fse_decompress.c:199-250): after each symbol's state
        // update, an exhausted stream ends with one more symbol from the other state
        uint32_t s1 = bb.get(al, lane), s2 = bb.get(al, lane);
        n = 0;
        for (int k = 0;; k ^= 1) {
            if (n > 253) return ZC;
            const Cell e = lds_cell(&L.wt[k ? s2 : s1]);
            if (lane == 0) L.weights[n] = (uint8_t)c_sym(e);
            n++;
            const uint32_t ns = c_next(e) + bb.get(c_nb(e), lane);
            if (k) s2 = ns; else s1 = ns;
            if (bb.left() < 0) {
                const Cell e2 = lds_cell(&L.wt[k ? s1 : s2]);
                if (lane == 0) L.weights[n] = (uint8_t)c_sym(e2);
                n++;
                break;
            }
        }
    }
    wave_lds_fence();
    // weights -> table log, the implied last weight (HUF_readStats: a clean power of 2 completes
    // the total), at least two and an even number of weight-1 symbols
    uint32_t total = 0;
    int c1 = 0;
    for (int i = 0; i < n; i++) {
        const int w = (int)lds_u8(&L.weights[i]);
        if (w > 12) return ZC;
        c1 += w == 1;
        total += (1u << w) >> 1;
    }
    if (total == 0) return ZC;
    tl = hb32(total) + 1;
    if (tl > 12) return ZC;
    if (tl > kHufLogMax) return kErrUnsupported;
    const uint32_t rest = (1u << tl) - total;
    if (rest & (rest - 1)) return ZC;
    const int lw = hb32(rest) + 1;
    if (lane == 0) L.weights[n] = (uint8_t)lw;
    c1 += lw == 1;
    n++;
    if (c1 < 2 || (c1 & 1)) return ZC;
    wave_lds_fence();
    // table (HUF_readDTableX1): weight 1 first, symbols in order within a weight, 2^(w-1) cells
    // each; symbols of a weight found by ballot over the 4 x 64 weights held in registers
    uint32_t wv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) wv[j] = lane + 64 * j < n ? (uint32_t)L.weights[lane + 64 * j] : 0u;
    int start = 0;
    for (int w = 1; w <= tl; w++) {
        const int len = 1 << (w - 1);
        const uint32_t cell = (uint32_t)(tl + 1 - w) << 8;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            for (uint64_t m = ballot(wv[j] == (uint32_t)w); m; m &= m - 1) {
                const uint32_t s = (uint32_t)(__builtin_ctzll(m) + 64 * j);
                for (int i = lane; i < len; i += LZH_WAVE) L.huf[start + i] = (uint16_t)(cell | s);
                start += len;
            }
        }
    }
    wave_lds_fence();
    return used;
}

// literals of one Huffman stream set into out[dst .. dst + rs): 1 or 4 streams (1X1 / 4X1,
// huf_decompress.c HUF_decompress1X1 / 4X1_usingDTable), one stream per lane.  Lane j holds
// stream j's backward bit container as in BackBits (64 bits c at bit offset D8, position P): a
// container refill always moves down by exactly one dword (P - tl < D8 happens only once P is
// within tl bits of D8), so the next dwords below are prefetched per lane, four at a time
// (bank a in use, bank b in flight); the symbol lookup is a per-lane LDS read and each step
// stores one byte per stream.  The streams' decoding chains run side by side in the lanes.
__device__ __forceinline__ int huf_streams(const Bytes& src, int pos, int csize, int nstreams, const Bytes& out, int dst, int rs,
                            int tl, LDSA Lds& L, int lane) {
    int seg = rs, last = rs, s0 = pos, sz = csize;   // this lane's stream: [s0, s0 + sz), seg (or last) symbols
    if (nstreams == 4) {
        if (csize < 10) return ZC;
        ZWin fw;
        fw.bind(src, nullptr);
        fw.load(pos, lane);
        const int z1 = (int)(fword(fw, pos, lane) & 0xffffu), z2 = (int)(fword(fw, pos + 2, lane) & 0xffffu),
                  z3 = (int)(fword(fw, pos + 4, lane) & 0xffffu);
        const int z4 = csize - 6 - z1 - z2 - z3;
        if (z4 < 1) return ZC;
        seg = (rs + 3) / 4;
        last = rs - 3 * seg;
        if (last < 0) return ZC;
        if (z1 <= 0 || z2 <= 0 || z3 <= 0) return ZC;
        const int p1 = pos + 6;
        s0 = lane == 0 ? p1 : (lane == 1 ? p1 + z1 : (lane == 2 ? p1 + z1 + z2 : p1 + z1 + z2 + z3));
        sz = lane == 0 ? z1 : (lane == 1 ? z2 : (lane == 2 ? z3 : z4));
    } else if (csize <= 0) {
        return ZC;
    }
    const bool on = lane < nstreams;
    const int nsym = lane == 3 ? last : seg;           // symbols of this lane's stream
    const rsrc_t r = src.r;
    const int x0 = s0 + src.sh;
    const int X = x0 + sz - 1;                          // the stream's last byte holds the end mark
    const uint32_t lastb = on ? ld_u8(r, X) : 1u;
    if (ballot(on && lastb == 0)) return ZC;
    const int lo = 8 * x0;
    int P = 8 * X + hb32(lastb);
    int D8 = ((P - 32) >> 5) << 5;
    int D = D8 >> 3;                                    // (dword aligned; below 0 reads as 0)
    uint64_t c = on ? (((uint64_t)ld_b32(r, D + 4) << 32) | ld_b32(r, D)) : 0ull;
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    if (on) {
        a0 = ld_b32(r, D - 4); a1 = ld_b32(r, D - 8); a2 = ld_b32(r, D - 12); a3 = ld_b32(r, D - 16);
        b0 = ld_b32(r, D - 20); b1 = ld_b32(r, D - 24); b2 = ld_b32(r, D - 28); b3 = ld_b32(r, D - 32);
    }
    int na = 4, nxt = D - 36;                           // dwords left in bank a; next dword to fetch
    const uint32_t mask = (1u << tl) - 1u;
    for (int i = 0; i < seg; i++) {
        const bool act = on && i < nsym;
        if (act && P - tl < D8) {                       // container refill: one dword down
            c = (c << 32) | a0;
            a0 = a1; a1 = a2; a2 = a3;
            D8 -= 32;
            if (--na == 0) {                            // bank b becomes a, the next four are fetched
                a0 = b0; a1 = b1; a2 = b2; a3 = b3;
                b0 = ld_b32(r, nxt); b1 = ld_b32(r, nxt - 4); b2 = ld_b32(r, nxt - 8); b3 = ld_b32(r, nxt - 12);
                nxt -= 16;
                na = 4;
            }
        }
        const int sh = P - tl - D8;
        uint32_t v = (uint32_t)(c >> (sh & 63)) & mask;
        if (P - tl < lo) v &= (uint32_t)(~0ull << min(lo - (P - tl), 63));   // zero-padded below the start
        const uint32_t e = ((volatile const LDSA uint16_t*)L.huf)[act ? v : 0];
        if (act) {
            P -= (int)(e >> 8);
            out.st8(dst + lane * seg + i, e & 0xffu);
        }
    }
    return ballot(on && P != lo) ? 1 : 0;              // 1: some stream not exactly consumed
}

// HUF_selectDecoder (huf_decompress.c:1565-1615): 1 when the reference decodes a 4-stream literal
// section it has just read a tree for with the double-symbol decoder (X2)
LZH_HDR_VAR __constant__ uint16_t kAlgoTime[16][4] = {
    {0, 0, 1, 1}, {0, 0, 1, 1}, {150, 216, 381, 119}, {170, 205, 514, 112}, {177, 199, 539, 110},
    {197, 194, 644, 107}, {221, 192, 735, 107}, {256, 189, 881, 106}, {359, 188, 1167, 109},
    {582, 187, 1570, 114}, {688, 187, 1712, 122}, {825, 186, 1965, 136}, {976, 185, 2131, 150},
    {1180, 186, 2070, 175}, {1377, 185, 1731, 202}, {1412, 185, 1695, 202}};
__device__ __forceinline__ bool huf_select_x2(int dstSize, int cSrcSize) {
    const int Q = cSrcSize >= dstSize ? 15 : (int)((uint32_t)cSrcSize * 16u / (uint32_t)dstSize);
    const uint32_t D256 = (uint32_t)dstSize >> 8;
    const uint32_t t0 = kAlgoTime[Q][0] + kAlgoTime[Q][1] * D256;
    uint32_t t1 = kAlgoTime[Q][2] + kAlgoTime[Q][3] * D256;
    t1 += t1 >> 5;
    return t1 < t0;
}

// The double-symbol decoder's verdict (HUF_decompress1X2 / 4X2_usingDTable_internal_body,
// huf_decompress.c:1176-1363), run when the single-symbol walk of huf_streams did not consume some
// stream exactly and the reference table is X2.  Both decoders emit the same symbols wherever the
// bits are read inside the stream (an X2 cell of targetLog = max(11, tl) bits holds the next code
// and, when both fit, the code after it: HUF_fillDTableX2), and a stream X1 accepts X2 accepts
// with the same bytes.  X2 differs on corrupt streams in three ways, restated here per lane (one
// stream per lane, lookups in lock step):
//  * the last symbol of a stream (HUF_decodeLastSymbolX2, :1148-1163): a two-symbol cell skips
//    both codes and clamps an overrun to the stream start, so the stream ends exactly consumed
//    whenever it had bits left; with none left the cell comes from the top bits of the 64-bit
//    container loaded at the stream start (bitsConsumed == 64: the shift wraps to 0);
//  * the 4-stream loop (:1294-1342) decodes 4 cells per stream per round, 1 or 2 symbols each,
//    until some stream's reload pointer is within 8 bytes of its start or stream 4 is within 7
//    bytes of its end; a stream 1..3 that wrote past its segment by then is corrupt (:1345-1347).
//    After a round's reload the pointer is ceil(r / 8) - 8 bytes above the stream start
//    (BIT_reloadDStreamFast, r = bits left), before the first one srcSize - 8 (or 0 below 8 bytes);
//  * anything consumed below the stream start is never recovered (bitsConsumed > 64), except by
//    the last-symbol clamp above.
// Symbols are written in place of the X1 walk's; returns 0 (accepted) or ZC.
__device__ __attribute__((noinline)) int huf_streams_x2(const Bytes& src, int pos, int csize, int nstreams, const Bytes& out,
                                                         int dst, int rs, int tl, LDSA Lds& L, int lane) {
    const rsrc_t r = src.r;
    int seg = rs, last = rs, s0 = pos, sz = csize;
    if (nstreams == 4) {                               // (geometry validated by huf_streams)
        const int b = pos + src.sh;
        const int z1 = (int)(ld_u8(r, b) | ld_u8(r, b + 1) << 8), z2 = (int)(ld_u8(r, b + 2) | ld_u8(r, b + 3) << 8),
                  z3 = (int)(ld_u8(r, b + 4) | ld_u8(r, b + 5) << 8);
        seg = (rs + 3) / 4;
        last = rs - 3 * seg;
        const int p1 = pos + 6;
        s0 = lane == 0 ? p1 : (lane == 1 ? p1 + z1 : (lane == 2 ? p1 + z1 + z2 : p1 + z1 + z2 + z3));
        sz = lane == 0 ? z1 : (lane == 1 ? z2 : (lane == 2 ? z3 : csize - 6 - z1 - z2 - z3));
    }
    const bool on = lane < nstreams;
    const int nsym = lane == 3 ? last : seg;
    const int x0 = s0 + src.sh, lo = 8 * x0, X = x0 + sz - 1;
    const uint32_t lastb = on ? ld_u8(r, X) : 1u;
    int P = 8 * X + hb32(lastb | 1u);
    const int T = tl <= 11 ? 11 : 12;                  // HUF_readDTableX2: maxTableLog, :1081
    const uint32_t tmask = (1u << T) - 1u;
    const uint32_t b6 = on && sz >= 7 ? ld_u8(r, x0 + 6) : 0u, b7 = on && sz >= 8 ? ld_u8(r, x0 + 7) : 0u;
    const uint32_t top = ((b7 << 8) | b6) >> (16 - T);   // BIT_initDStream's container, top T bits
    int q = sz >= 8 ? sz - 8 : 0;                      // reload pointer - start, bytes
    bool joint = nstreams == 4 && last >= 8;           // (oend - op4 >= 8 and op4 < olimit)
    int op = 0;
    for (int t = 0;; t++) {
        if (joint && t > 0 && (t & 3) == 0) {          // end of a round: the four reloads, the loop test
            const bool cont = q >= 8 && !(lane == 3 && op >= last - 7);
            if (ballot(on && !cont)) {
                joint = false;
                if (ballot(on && lane < 3 && op > seg)) return ZC;
            } else {
                q = ((P - lo + 7) >> 3) - 8;
            }
        }
        const bool act = on && (joint || op < nsym);
        if (!ballot(act)) break;
        if (!act) continue;
        uint32_t v;
        if (P == lo) {
            v = top;
        } else {
            const int qb = (P - T) >> 3, sh = (P - T) & 7;
            const uint32_t w = ld_u8(r, qb) | ld_u8(r, qb + 1) << 8 | ld_u8(r, qb + 2) << 16;
            v = (w >> sh) & tmask;
            if (P - T < lo) v &= (uint32_t)(~0ull << min(lo - (P - T), 32));   // zero-padded below the start
        }
        const uint32_t e1 = ((volatile const LDSA uint16_t*)L.huf)[v >> (T - tl)];
        const int n1 = (int)(e1 >> 8);
        const uint32_t e2 = ((volatile const LDSA uint16_t*)L.huf)[((v << n1) & tmask) >> (T - tl)];
        const int n2 = (int)(e2 >> 8);
        const bool dbl = n1 + n2 <= T;
        if (op < nsym) out.st8(dst + lane * seg + op, e1 & 0xffu);
        if (!joint && op == nsym - 1) {                // HUF_decodeLastSymbolX2
            if (!dbl) P -= n1;
            else if (P > lo) P = max(P - n1 - n2, lo);
            op++;
        } else {
            if (dbl && op + 1 < nsym) out.st8(dst + lane * seg + op + 1, e2 & 0xffu);
            P -= dbl ? n1 + n2 : n1;
            op += dbl ? 2 : 1;
        }
    }
    return ballot(on && P != lo) ? ZC : 0;
}

struct FrameState {
    int rep0, rep1, rep2;
    int llA, ofA, mlA;                  // accuracy logs of the current tables
    bool llV, ofV, mlV, hufV;           // tables valid for "repeat" / treeless modes
    bool hufX2;                         // the reference's table type (HUF_DTable tableType: 1 = X2)
    int hufTl;
    uint64_t clk[kZClk], clk_last;      // (LZH_ZSTD_STATS)
};

// The second match source of the dictionary calls (zstd_dict_hip.hip: a type with kOn = true, `bytes` and copy()).
// NoDict: none -- every use below is a compile-time constant and the decoders of this file keep their code.
struct NoDict {
    static constexpr bool kOn = false;
    static constexpr int bytes = 0;
};

// one compressed block [bs, be) of the frame; output continues at op (returns new op, < 0 error)
template <class DictT = NoDict>
__device__ __forceinline__ int decode_block(const Bytes& rin, const Bytes& lout, ZWin& fw, ZWin& lw, ZSink& O, LDSA Lds& L,
                            FrameState& F, int bs, int be, int op, int fcs, int lane, const DictT& D = DictT()) {
    // ---- literals section (ZSTD_decodeLiteralsBlock)
    const uint32_t b0 = fbyte(fw, bs, lane);
    const int ltype = (int)(b0 & 3u), sf = (int)((b0 >> 2) & 3u);
    int rs, lpos, seqpos;
    Bytes lsrc;                                       // where the literals are read from
    if (ltype <= 1) {
        int hsz;
        if ((sf & 1) == 0) { hsz = 1; rs = (int)(b0 >> 3); }
        else if (sf == 1) { hsz = 2; rs = (int)((b0 >> 4) + (fbyte(fw, bs + 1, lane) << 4)); }
        else { hsz = 3; rs = (int)((b0 >> 4) + (fbyte(fw, bs + 1, lane) << 4) + (fbyte(fw, bs + 2, lane) << 12)); }
        if (rs > kBlockMax) return ZC;
        if (ltype == 0) {
            if (bs + hsz + rs > be) return ZC;
            lsrc = rin;
            lpos = bs + hsz;
            seqpos = bs + hsz + rs;
        } else {
            if (bs + hsz + 1 > be || rs > fcs - op) return ZC;
            const uint32_t v = fbyte(fw, bs + hsz, lane);
            lsrc = lout;
            lpos = fcs - rs;
            for (int i = lane; i < rs; i += LZH_WAVE) O.out.st8(lpos + i, v);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            seqpos = bs + hsz + 1;
        }
    } else {
        const int hsz = sf <= 1 ? 3 : (sf == 2 ? 4 : 5);
        const int bits = sf <= 1 ? 10 : (sf == 2 ? 14 : 18);
        if (bs + hsz > be) return ZC;
        uint64_t h = 0;
        for (int i = 0; i < hsz; i++) h |= (uint64_t)fbyte(fw, bs + i, lane) << (8 * i);
        rs = (int)((h >> 4) & ((1u << bits) - 1));
        const int cs = (int)((h >> (4 + bits)) & ((1u << bits) - 1));
        if (rs > kBlockMax || bs + hsz + cs > be || rs > fcs - op) return ZC;
        int p = bs + hsz;
        if (ltype == 2) {
            int tl = 0;
            ZCLK(F, 0);
            const int u = read_huf(fw, rin, p, bs + hsz + cs, L, tl, lane);
            ZCLK(F, 1);
            if (u < 0) return u;
            F.hufV = true;
            F.hufTl = tl;
            // (ZSTD_decodeLiteralsBlock: a 1-stream tree is read as X1, a 4-stream one by HUF_selectDecoder)
            F.hufX2 = sf != 0 && huf_select_x2(rs, cs);
            p += u;
        } else if (!F.hufV) {
            return ZC;
        }
        lsrc = lout;
        lpos = fcs - rs;
        ZCLK(F, 0);
        if (rs == 0 && sf != 0 && ltype == 2) return ZC;   // HUF_decompress4X_hufOnly: dstSize 0
        int hr = huf_streams(rin, p, bs + hsz + cs - p, sf == 0 ? 1 : 4, O.out, lpos, rs, F.hufTl, L, lane);
        if (hr == 1)
            hr = F.hufX2 ? huf_streams_x2(rin, p, bs + hsz + cs - p, sf == 0 ? 1 : 4, O.out, lpos, rs, F.hufTl, L, lane) : ZC;
        ZCLK(F, 2);
        if (hr < 0) return hr;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // literal stores visible to the window loads
        seqpos = bs + hsz + cs;
    }
    lw.bind(lsrc, nullptr);
    lw.load(lpos, lane);

    // ---- sequences section header (ZSTD_decodeSeqHeaders)
    if (seqpos >= be) return ZC;
    int p = seqpos;
    int nseq = (int)fbyte(fw, p++, lane);
    if (nseq >= 128) {
        if (nseq == 255) {
            if (p + 2 > be) return ZC;
            nseq = (int)(fbyte(fw, p, lane) + (fbyte(fw, p + 1, lane) << 8)) + 0x7F00;
            p += 2;
        } else {
            if (p + 1 > be) return ZC;
            nseq = ((nseq - 128) << 8) + (int)fbyte(fw, p++, lane);
        }
    }
    int lp = 0;                                       // literals consumed
    if (nseq > 0) {
        if (p >= be) return ZC;
        const uint32_t modes = fbyte(fw, p++, lane);
        // (the two reserved bits: zstd 1.5.2's ZSTD_decodeSeqHeaders does not look at them; the decoders of this file
        // have always refused them and keep doing so, the dictionary decoder gives the reference's verdict)
        if (!DictT::kOn && (modes & 3u)) return ZC;
        ZCLK(F, 0);
        int u = seq_table(fw, p, be, (int)(modes >> 6), 0, L.ll, F.llA, F.llV, L, lane);
        if (u < 0) return ZC;
        p += u;
        u = seq_table(fw, p, be, (int)((modes >> 4) & 3u), 1, L.of, F.ofA, F.ofV, L, lane);
        if (u < 0) return ZC;
        p += u;
        u = seq_table(fw, p, be, (int)((modes >> 2) & 3u), 2, L.ml, F.mlA, F.mlV, L, lane);
        if (u < 0) return ZC;
        p += u;
        // ---- sequences (ZSTD_decodeSequence), executed a group at a time.  The decoding chain
        // (bit reader, FSE states, repcodes, lengths, the group being filled) lives in vector
        // registers (every lane holds the same value: vgpr() hides the uniformity from the
        // compiler), so the frame's scalar state is not spilled to VGPR lanes and back around
        // every sequence; table lookups are LDS reads at one address per wave.
        ZCLK(F, 3);
        SeqBits sb;
        if (!sb.init(rin, p, be - p)) return ZC;
        uint32_t sLL = sb.get(F.llA), sOF = sb.get(F.ofA), sML = sb.get(F.mlA);
        int rep0 = vgpr(F.rep0), rep1 = vgpr(F.rep1), rep2 = vgpr(F.rep2);
        int k = vgpr(0), glit = vgpr(0), gout = vgpr(0);   // group: members, literal bytes, output bytes
        const int lrem0 = vgpr(rs - lp), opv = vgpr(op), fcsv = vgpr(fcs);
        uint32_t g_lit = 0, g_ml = 0, g_off = 0, g_ex = 0, g_lrel = 0;
        const volatile LDSA uint32_t* llT = (const volatile LDSA uint32_t*)L.ll;
        const volatile LDSA uint32_t* mlT = (const volatile LDSA uint32_t*)L.ml;
        const volatile LDSA uint32_t* ofT = (const volatile LDSA uint32_t*)L.of;
        int lpv = 0, opg = 0;                         // literals / output bytes of the groups emitted
        for (int i = 0; i < nseq; i++) {
            const Cell eL = llT[sLL], eO = ofT[sOF], eM = mlT[sML];
            const int ofc = (int)c_sym(eO);
            const int llc = (int)c_sym(eL), mlc = (int)c_sym(eM);
            const int ll0 = llc == 0;                 // (only literal-length code 0 has baseline 0)
            int off;
            if (ofc > 1) {
                off = (int)((1u << ofc) - 3u + sb.get(ofc));
                rep2 = rep1; rep1 = rep0; rep0 = off;
            } else if (ofc == 0) {
                off = ll0 ? rep1 : rep0;
                if (ll0) { rep1 = rep0; rep0 = off; }
            } else {
                const int idx = 1 + ll0 + (int)sb.get(1);   // 1..3
                int t = idx == 3 ? rep0 - 1 : (idx == 1 ? rep1 : rep2);
                t += t == 0;                          // (as the reference: offset 0 becomes 1)
                if (idx != 1) rep2 = rep1;
                rep1 = rep0;
                rep0 = off = t;
            }
            // match-length then literal-length extra bits (<= 16 each), one read of both
            const int am = c_add(eM), al = c_add(eL);
            const uint32_t xb = sb.get(am + al);
            const int ml = (int)L.base[36 + mlc] + (int)(xb >> al);
            const int ll = (int)L.base[llc] + (int)(xb & ((1u << al) - 1u));
            if (i + 1 < nseq) {                       // state updates LL, ML, OF: one read (<= 27 bits)
                const int nl = c_nb(eL), nm = c_nb(eM), no = c_nb(eO);
                const uint32_t sbits = sb.get(nl + nm + no);
                sLL = c_next(eL) + (sbits >> (nm + no));
                sML = c_next(eM) + ((sbits >> no) & ((1u << nm) - 1u));
                sOF = c_next(eO) + (sbits & ((1u << no) - 1u));
                if (sb.left() < 0) return ZC;
            } else {
                // the reference also updates the states after the last sequence and then accepts
                // an exhausted or overrun stream (ZSTD_decompressSequences_body: reload >= completed)
                const int extra = c_nb(eL) + c_nb(eM) + c_nb(eO);
                if (sb.left() > extra || sb.left() < 0) return ZC;
            }
            // validity (ZSTD_execSequence): literals available, offset within the output, room
            const int lrem = lrem0 - lpv - glit;      // literals not yet taken
            const int o0 = opv + opg + gout;          // output position of this sequence
            // (an offset code of 31 gives 2^31 - 3 + bits: compared unsigned, as the reference's size_t)
            bool far = false;                         // (dictionary calls: the match starts before the output)
            if constexpr (DictT::kOn) {
                far = (uint32_t)off > (uint32_t)(o0 + ll);
                if (ll > lrem || (uint32_t)off > (uint32_t)(o0 + ll) + (uint32_t)D.bytes ||
                    (int64_t)o0 + ll + ml > (int64_t)(fcsv - (lrem - ll)))
                    return ZC;
            } else {
            if (ll > lrem || (uint32_t)off > (uint32_t)(o0 + ll) || (int64_t)o0 + ll + ml > (int64_t)(fcsv - (lrem - ll)))
                return ZC;
            }
            const bool big = ll > 255 || ml > 4095 || far;
            if (big || k == LZH_WAVE || glit + ll > 384) {
                // emit the pending group
                if (k > 0) {
                    const int kk = unii(k), gl = unii(glit), go = unii(gout), lpu = unii(lpv), opu = unii(op + opg);
                    const int ip = lpos + lp + lpu;
                    if (!lw.covers(ip, ip + gl + 16)) lw.load(ip, lane);
                    const uint64_t keep = kk == LZH_WAVE ? ~0ull : ((1ull << kk) - 1ull);
                    ZCLK(F, 4);
                    groups::emit_group(lw, O, (LDSA uint8_t*)L.win + kZW, ip, opu, go, keep, (int)g_ex,
                                       g_lit | (g_ml << 16), g_lrel, (int)g_off, lane);
                    ZCLK(F, 5);
                    opg += gout;
                    lpv += glit;
                    k = 0; glit = 0; gout = 0;
                }
                if (big) {                            // a long sequence on its own
                    const int bl = unii(ll), bm = unii(ml), bo = unii(off), lpu = unii(lpv), opu = unii(op + opg);
                    ZCLK(F, 4);
                    O.literals(lw, lsrc, lpos + lp + lpu, opu, bl, lane);
                    if constexpr (DictT::kOn) {
                        // dictionary bytes first, then the output's own from its first byte on
                        const int back = bo - (opu + bl), dn = back > 0 ? min(back, bm) : 0;
                        if (dn > 0) D.copy(O, opu + bl, back, dn, lane);
                        if (bm > dn) O.match(opu + bl + dn, bo, bm - dn, lane);
                    } else {
                    O.match(opu + bl, bo, bm, lane);
                    }
                    ZCLK(F, 6);
                    opg += ll + ml;
                    lpv += ll;
                    continue;
                }
            }
            g_lit = lane == k ? (uint32_t)ll : g_lit;
            g_ml = lane == k ? (uint32_t)ml : g_ml;
            g_off = lane == k ? (uint32_t)off : g_off;
            g_ex = lane == k ? (uint32_t)gout : g_ex;
            g_lrel = lane == k ? (uint32_t)glit : g_lrel;
            k++;
            glit += ll;
            gout += ll + ml;
        }
        if (unii(k) > 0) {
            const int kk = unii(k), gl = unii(glit), go = unii(gout), lpu = unii(lpv), opu = unii(op + opg);
            const int ip = lpos + lp + lpu;
            if (!lw.covers(ip, ip + gl + 16)) lw.load(ip, lane);
            const uint64_t keep = kk == LZH_WAVE ? ~0ull : ((1ull << kk) - 1ull);
            ZCLK(F, 4);
            groups::emit_group(lw, O, (LDSA uint8_t*)L.win + kZW, ip, opu, go, keep, (int)g_ex, g_lit | (g_ml << 16),
                               g_lrel, (int)g_off, lane);
            ZCLK(F, 5);
            opg += gout;
            lpv += glit;
        }
        op += unii(opg);
        lp += unii(lpv);
        F.rep0 = unii(rep0); F.rep1 = unii(rep1); F.rep2 = unii(rep2);
    } else if (p != be) {
        return ZC;
    }
    // last literals
    const int rem = rs - lp;
    if (rem > 0) {
        if (rem > fcs - op) return ZC;
        O.literals(lw, lsrc, lpos + lp, op, rem, lane);
        op += rem;
    }
    return op;
}

// one frame in rin[0, cs) -> out[0, cap): returns the decoded size or an error code
// lout: the output region for reading decoded literals back (whole dwords: its range ends at
// the dword holding the last byte, so no load that straddles the end reads back as zero)
template <class DictT = NoDict>
__device__ __forceinline__ int decode_frame(const Bytes& rin, const Bytes& lout, int cs, ZSink& O, LDSA Lds& L, int cap,
                            int lane, unsigned long long* stats, const DictT& D = DictT()) {
    ZWin fw;
    fw.bind(rin, nullptr);
    fw.load(0, lane);
    if (cs < 9) return ZC;
    const uint32_t magic = fword(fw, 0, lane);
    if (magic != 0xFD2FB528u) return (magic & 0xFFFFFFF0u) == 0x184D2A50u ? kErrUnsupported : kErrCorrupt;
    const uint32_t fhd = fbyte(fw, 4, lane);
    const int fcsf = (int)(fhd >> 6), single = (int)((fhd >> 5) & 1u);
    if (fhd & 8u) return ZC;                  // reserved bit
    const int ccrc = (fhd & 4u) ? 4 : 0;      // content checksum: XXH64 low 32 bits after the last block
    int p = 5;
    if (!single) {
        const uint32_t wd = fbyte(fw, p++, lane);
        if ((wd >> 3) + 10 > 27) return kErrUnsupported;   // window beyond the reference's default limit
    }
    const int dsz = (int)(fhd & 3u) == 3 ? 4 : (int)(fhd & 3u);
    uint32_t dict = 0;
    for (int i = 0; i < dsz; i++) dict |= fbyte(fw, p + i, lane) << (8 * i);
    p += dsz;
    if (dict) return kErrUnsupported;
    const int fsz = fcsf == 0 ? (single ? 1 : 0) : (fcsf == 1 ? 2 : (fcsf == 2 ? 4 : 8));
    if (fsz == 0) return kErrUnsupported;              // content size absent
    uint64_t fcs = 0;
    for (int i = 0; i < fsz; i++) fcs |= (uint64_t)fbyte(fw, p + i, lane) << (8 * i);
    if (fsz == 2) fcs += 256;
    p += fsz;
    if (fcs > (uint64_t)cap) return ZC;
    const int n = (int)fcs;
    FrameState F{1, 4, 8, 0, 0, 0, false, false, false, false, false, 0, {0, 0, 0, 0, 0, 0, 0, 0}, 0};
    if (LZH_ZSTD_STATS) F.clk_last = __builtin_amdgcn_s_memtime();
    ZWin lw;
    lw.bind(rin, nullptr);
    lw.load(0, lane);
    int op = 0;
    for (int guard = 0; guard <= cs; guard++) {
        if (p + 3 > cs) return ZC;
        const uint32_t bh = fbyte(fw, p, lane) | (fbyte(fw, p + 1, lane) << 8) | (fbyte(fw, p + 2, lane) << 16);
        p += 3;
        const int last = (int)(bh & 1u), type = (int)((bh >> 1) & 3u), bsz = (int)(bh >> 3);
        if (bsz > kBlockMax) return ZC;
        if (type == 0) {
            if (p + bsz > cs || bsz > n - op) return ZC;
            O.literals(fw, rin, p, op, bsz, lane);
            op += bsz;
            p += bsz;
        } else if (type == 1) {
            if (p + 1 > cs || bsz > n - op) return ZC;
            const uint32_t v = fbyte(fw, p, lane);
            for (int base = 0; base < bsz; base += LZH_WAVE) {
                if (base + lane < bsz) O.put(op + base + lane, v);
                O.maybe_flush(op + min(base + LZH_WAVE, bsz), lane);
            }
            op += bsz;
            p += 1;
        } else if (type == 2) {
            if (p + bsz > cs) return ZC;
            const int r = decode_block(rin, lout, fw, lw, O, L, F, p, p + bsz, op, n, lane, D);
            if (r < 0) return r;
            op = r;
            p += bsz;
        } else {
            return ZC;
        }
        if (last) break;
    }
    ZCLK(F, 7);
    if (LZH_ZSTD_STATS && stats && lane == 0)
        for (int i = 0; i < kZClk; i++) atomicAdd(&stats[i], (unsigned long long)F.clk[i]);
    if (op != n || p + ccrc != cs) return ZC;
    if (ccrc) {   // ZSTD_decompressFrame's checksum check (zstd_decompress.c:1011-1020), once the output is out
        O.flush(op, lane);
        wait_vm();
        const uint32_t want = fword(fw, p, lane);
        if ((uint32_t)xxh64_wave(O.out, op, lane) != want) return kErrChecksum;
        O.flushed = op;
    }
    return op;
}

}  // namespace zstdd
#ifndef LZH_ZSTD_MINW   // (lzh_zstd_decompress_kernel and its ragged and dictionary forms)
#define LZH_ZSTD_MINW 1   // waves per SIMD the register allocation must allow (LDS allows 3)
#endif
