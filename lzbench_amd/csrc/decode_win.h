// lzbench_amd/csrc/decode_win.h -- what every decoder here is built on: the register window over the compressed
// stream (WinT), the LDS output window (owin::SinkT) and the group emitter through it (groups::emit_group).
#pragma once
// (device variables of the decoder's headers: internal to a unit; external in decode_hip.hip, which defines this empty
// before its first include.  A second unit doing so would define the same external symbols twice: a link error)
#ifndef LZH_HDR_VAR
#define LZH_HDR_VAR static
#endif
#include "common.h"

// Debug counters (-DLZH_DEC_STATS=1 builds only, read by tools/dec_stats.py): per-wave sums in LDS,
// added to a device array when the chunk ends.
#ifndef LZH_DEC_STATS
#define LZH_DEC_STATS 0
#endif
#if LZH_DEC_STATS
__shared__ unsigned long long g_dst[16];
LZH_HDR_VAR __device__ unsigned long long lzh_dec_stats_buf[16];
#define DST(i, v) do { if (threadIdx.x == 0) g_dst[i] += (unsigned long long)(v); } while (0)
#define DCLK(t) const uint64_t t = __builtin_amdgcn_s_memtime()
#else
#define DST(i, v) do {} while (0)
#define DCLK(t) do {} while (0)
#endif
#ifdef LZH_ISA_MARKS
#define DMARK(i) asm volatile("; DMARK " #i ::: "memory")
#else
#define DMARK(i) ((void)0)
#endif

namespace {

constexpr int kRingBytes = 512 + 16;   // LDS copy of a window: ring over offsets mod 512 + mirror

// Register window over a byte stream (512 bytes in two VGPRs across the wave) with an LDS copy
// (ring indexed by descriptor offset mod 512, its first 16 bytes mirrored past the end): uniform
// reads use v_readlane on the registers, per-lane reads one LDS load instead of cross-lane
// permutes of both registers.
template <bool kRing>
struct WinT {
    rsrc_t r;
    int sh;       // descriptor offset of stream byte 0
    int wb;       // descriptor offset (4-aligned) of the window start
    uint32_t w0, w1;
    LDSA uint8_t* ring;
    __device__ __forceinline__ void bind(const Bytes& b, LDSA uint8_t* rg) { r = b.r; sh = b.sh; ring = rg; }
    __device__ __forceinline__ void put_ring(int D, uint32_t v) const {
        if (!kRing) return;
        const int i = D & 511;
        *(volatile LDSA uint32_t*)(ring + i) = v;
        if (i < 16) *(volatile LDSA uint32_t*)(ring + 512 + i) = v;
    }
    __device__ __forceinline__ void load(int pos, int lane) {
        wb = (pos + sh) & ~3;
        w0 = ld_b32(r, wb + 4 * lane);
        w1 = ld_b32(r, wb + 256 + 4 * lane);
        put_ring(wb + 4 * lane, w0);
        put_ring(wb + 256 + 4 * lane, w1);
    }
    // make stream bytes [pos, pos+16) addressable
    __device__ __forceinline__ void ensure(int pos, int lane) {
        const int x = pos + sh;
        if (x >= wb && x + 16 <= wb + 512) return;
        if (x >= wb + 256 && x + 16 <= wb + 768) {
            w0 = w1;
            wb += 256;
            w1 = ld_b32(r, wb + 256 + 4 * lane);
            put_ring(wb + 256 + 4 * lane, w1);
            return;
        }
        load(pos, lane);
    }
    __device__ __forceinline__ uint32_t byte(int pos) const {
        const int x = pos + sh;
        const int d = (x - wb) >> 2;
        const uint32_t v = d < 64 ? rdlane(w0, d) : rdlane(w1, d - 64);
        return (v >> (8 * (x & 3))) & 0xffu;
    }
    __device__ __forceinline__ bool covers(int p0, int p1) const { return p0 + sh >= wb && p1 + sh <= wb + 512; }
    // per-lane 4 bytes at stream position pos (pos .. pos+3 inside the window)
    __device__ __forceinline__ uint32_t lane_word(int pos) const {
        const int x = pos + sh;
        if (kRing) {
            const int a = x & 508;
            const uint32_t lo = *(volatile const LDSA uint32_t*)(ring + a), hi = *(volatile const LDSA uint32_t*)(ring + a + 4);
            return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)x & 3u);
        }
        const int d = (x - wb) >> 2;
        const uint32_t a0 = lane_gather(w0, d & 63), a1 = lane_gather(w1, d & 63);
        const uint32_t b0 = lane_gather(w0, (d + 1) & 63), b1 = lane_gather(w1, (d + 1) & 63);
        const uint32_t lo = d < 64 ? a0 : a1, hi = d + 1 < 64 ? b0 : b1;
        return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)x & 3u);
    }
    // per-lane byte at stream position pos (inside the window) via cross-lane permute
    __device__ __forceinline__ uint32_t lane_byte(int pos) const {
        const int x = pos + sh;
        if (kRing) return ((volatile const LDSA uint8_t*)ring)[x & 511];
        const int d = (x - wb) >> 2;
        const uint32_t a = lane_gather(w0, d & 63), b = lane_gather(w1, d & 63);
        return ((d < 64 ? a : b) >> (8 * (x & 3))) & 0xffu;
    }
};

typedef WinT<true> Win;     // lz4 / snappy decoders
typedef WinT<false> ZWin;   // zstd (its LDS budget has no room for rings: 8 waves per CU)

__device__ __forceinline__ void copy_raw(const Bytes& in, const Bytes& out, int len, int lane) {
    copy_span(in, 0, out, 0, len, lane, LZH_WAVE);
}

}  // namespace

// ---------------------------------------------------------------------------------------
// Output through an LDS window.  The last kW decoded bytes of the chunk stay in LDS, so a
// match whose source lies in them is an LDS-to-LDS copy with no memory round trip; decoded
// bytes leave for global memory as aligned dword stores once 256 are pending.  Far matches read
// the (already flushed) output with L1-bypassing loads.
namespace owin {

#ifndef LZH_DEC_KW
#define LZH_DEC_KW 4096
#endif
#ifndef LZH_DEC_WIDE
#define LZH_DEC_WIDE 2   // wider output windows for launches with few chunks: 0 off, 1 up to 8 KiB, 2 up to 16 KiB
#endif
constexpr int kW = LZH_DEC_KW;   // LDS output window bytes (power of two)

template <int KW>
struct SinkT {
    static constexpr int kWin = KW;
    LDSA uint8_t* b;
    Bytes out;
    int flushed;      // output bytes [0, flushed) are in global memory
    int ringlo;       // output bytes [ringlo, op) are in the window (bulk literal runs bypass it)
    __device__ __forceinline__ void put(int pos, uint32_t v) const {
        ((volatile LDSA uint8_t*)b)[(pos + out.sh) & (KW - 1)] = (uint8_t)v;
    }
    __device__ __forceinline__ uint32_t get(int pos) const {
        return ((volatile const LDSA uint8_t*)b)[(pos + out.sh) & (KW - 1)];
    }
    __device__ __forceinline__ uint32_t dword(int X) const {
        return ((volatile const LDSA uint32_t*)b)[(X & (KW - 1)) >> 2];
    }
    // global <- window bytes [flushed, upto)
    __device__ __forceinline__ void flush(int upto, int lane) {
        const int fx = flushed + out.sh, ux = upto + out.sh;
        for (int D0 = fx & ~3; D0 < ux; D0 += 4 * LZH_WAVE) {
            const int D = D0 + 4 * lane;
            const uint32_t w = dword(D);
            if (D >= fx && D + 4 <= ux) {
                st_b32(out.r, D, w);
            } else if (D + 4 > fx && D < ux) {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (D + k >= fx && D + k < ux) st_u8(out.r, D + k, (w >> (8 * k)) & 0xffu);
            }
        }
        flushed = upto;
    }
    __device__ __forceinline__ void maybe_flush(int op, int lane) {
        if (op - flushed >= 4 * LZH_WAVE) flush(((op + out.sh) & ~3) - out.sh, lane);
    }

    // literal run in[src, src+len) -> op
    template <class W>
    __device__ __forceinline__ void literals(const W& w, const Bytes& in, int src, int op, int len, int lane) {
        if (len > 8 * LZH_WAVE) {
            // bulk: straight to global memory; the window restarts after the run
            flush(op, lane);
            copy_span(in, src, out, op, len, lane, LZH_WAVE);
            flushed = op + len;
            ringlo = op + len;
            return;
        }
        for (int base = 0; base < len; base += LZH_WAVE) {
            const int t = base + lane;
            uint32_t v;
            if (w.covers(src + base, src + base + LZH_WAVE)) v = w.lane_byte(src + t);
            else v = in.b(src + t);
            if (t < len) put(op + t, v);
            maybe_flush(op + min(base + LZH_WAVE, len), lane);
        }
    }

    // out[op + t] = out[op - off + t] for t < len (byte by byte semantics), 0 < off <= op
    __device__ __forceinline__ void match(int op, int off, int len, int lane) {
        const int src0 = op - off;
        // (reach kWin - 128: the group emitter may have written up to 127 bytes past its end)
        if (src0 >= ringlo && off <= KW - 2 * LZH_WAVE) {
            // (a period shorter than the wave: the first `per` bytes come from the period before op, the rest
            // from this match's own output `per` bytes back -- a multiple of the period of at least a wave, so
            // written by an earlier round and still in the window however long the match is)
            const int per = off >= LZH_WAVE ? off : off * ((LZH_WAVE + off - 1) / off);
            for (int base = 0; base < len; base += LZH_WAVE) {
                const int t = base + lane;
                const int s = off >= LZH_WAVE ? src0 + t
                            : (t < per ? src0 + (int)((uint32_t)t % (uint32_t)off) : op + t - per);
                const uint32_t v = get(s);
                if (t < len) put(op + t, v);
                maybe_flush(op + min(base + LZH_WAVE, len), lane);
            }
            return;
        }
        // far: the source is in global memory once every pending byte is flushed and stored
        flush(op, lane);
        for (int base = 0; base < len; base += LZH_WAVE) {
            const int t = base + lane;
            const int s = off >= LZH_WAVE ? src0 + t : src0 + (int)((uint32_t)t % (uint32_t)off);
            if (off < len && base > 0) flush(op + base, lane);   // sources in this match's output
            else maybe_flush(op + base, lane);   // (a match longer than the window must not wrap it while pending)
            wait_vm();
            const uint32_t v = t < len ? out.b_sc1(s) : 0u;
            if (t < len) put(op + t, v);
        }
        maybe_flush(op + len, lane);
    }
};

typedef SinkT<kW> Sink;

}  // namespace owin

// The group emitter (the LZ4 / snappy group decoders of decode_hip.hip and the zstd decoders end in it).
namespace groups {

__device__ __forceinline__ int wave_incl_scan(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return x;
}

// Output byte ob (group-relative) from its owner's fields, precomputed per member so that a byte
// costs adds and compares only: lend = the owner's literal end (group-relative), lsb = stream
// position of its literal byte at ob = lsb + ob, msrc = absolute output position of its match
// source at ob = msrc + ob (byte-by-byte semantics; overlapping copies take the period form).
// done = final now (not an unresolved in-pass source); far = source only in global memory.
template <class W, class SinkType>
__device__ __forceinline__ uint32_t owned_byte(const W& w, const SinkType& O, int op, int pbase, int thr, int ob,
                                               int total, int lend, int lsb, int msrc, int offk, int& src,
                                               uint64_t& done, uint64_t& far) {
    // (lane masks from single-compare ballots: a ballot of a compound bool goes through a VGPR)
    const uint64_t il = ballot(ob < lend), act = ballot(ob < total);
    const bool is_lit = lane_on(il);
    const uint32_t lb = w.lane_byte(lsb + (is_lit ? ob : lend - 1));
    src = msrc + ob;
    const uint64_t ov = ballot(ob >= lend + offk) & ~il;
    if (ov & act) {                                                // overlapping copy: period offk
        const int md = (int)((uint32_t)(ob - lend) % (uint32_t)max(offk, 1));
        src = lane_on(ov) ? op + lend - offk + md : src;
    }
    const uint32_t g = O.get(src);
    const uint64_t near = ballot(src >= O.ringlo) & ballot(src >= thr) & ~il;
    const uint64_t inpass = ballot(src >= pbase) & ~il;
    done = il | (near & ~inpass);
    far = act & ~il & ~near;
    return is_lit ? lb : g;
}

// The part of a 128-byte pass after its far reads are issued (their data are used here first):
// store the bytes, resolve in-pass sources in dependency rounds, flush.
struct Tail {
    uint64_t far0, far1, done0, done1;   // (lane masks)
    uint32_t v0, v1, g0, g1;
    int src0, src1, ob0, ob1, pbase, op, total;
};

template <class SinkType>
__device__ __forceinline__ void pass_tail(SinkType& O, Tail& t, int lane) {
    constexpr int kP = 2 * LZH_WAVE;
    const uint32_t v0 = lane_on(t.far0) ? t.g0 : t.v0, v1 = lane_on(t.far1) ? t.g1 : t.v1;
    const int op = t.op, pbase = t.pbase, ob0 = t.ob0, ob1 = t.ob1, src0 = t.src0, src1 = t.src1;
    // (bytes past the group's end land in window slots at most 127 bytes past it, which no
    // later reader takes as near: the next group's threshold, SinkT::match's kWin - 128 reach)
    O.put(op + ob0, v0);
    O.put(op + ob1, v1);
    // in-pass sources: rounds until every byte read a finished source
    uint64_t dm0 = t.done0 | t.far0 | ballot(ob0 >= t.total), dm1 = t.done1 | t.far1 | ballot(ob1 >= t.total);
    uint32_t w0 = v0, w1 = v1;
    for (int r = 0; r < kP && (~dm0 | ~dm1); r++) {
        DST(4, 1);
        const int s0 = src0 - pbase, s1 = src1 - pbase;
        // (the lanes that read a finished source, as masks: one compare per ballot -- a ballot of the compound
        // bool goes through a VGPR)
        const uint64_t rm0 = ballot((((s0 & 1 ? dm1 : dm0) >> ((s0 >> 1) & 63)) & 1ull) != 0ull) & ~dm0;
        const uint64_t rm1 = ballot((((s1 & 1 ? dm1 : dm0) >> ((s1 >> 1) & 63)) & 1ull) != 0ull) & ~dm1;
        const bool rd0 = lane_on(rm0), rd1 = lane_on(rm1);
        const uint32_t q0 = O.get(src0), q1 = O.get(src1);
        w0 = rd0 ? q0 : w0;
        w1 = rd1 ? q1 : w1;
        O.put(op + ob0, w0);
        O.put(op + ob1, w1);
        dm0 |= rm0;
        dm1 |= rm1;
    }
    O.maybe_flush(min(pbase + kP, op + t.total), lane);
}

// Two output bytes per lane per pass (128-byte passes): a byte pair has at most two owners (the
// member owning its first byte, and one starting at its second), so each pass gathers two sets of
// member fields instead of one per 64 bytes.  Marks: 128 bytes + 64 bytes of scratch.
template <class W, class SinkType>
__device__ __forceinline__ void emit_group(const W& w, SinkType& O, LDSA uint8_t* mark, int ip, int op,
                                           int total, uint64_t keep, int excl, uint32_t pA, uint32_t lrel,
                                           int off, int lane) {
    constexpr int kP = 2 * LZH_WAVE;
    const bool kmem = lane_on(keep);
    int carry = 63 - __builtin_clzll(keep);                      // (pass 0 always has a start at 0)
    // per member: literal end, literal stream base, match source base (see owned_byte)
    const int m_lend = excl + (int)(pA & 0xffffu);
    const int m_lsb = ip + (int)lrel - excl;
    const int m_msrc = op - off;
    const uint64_t below = (1ull << lane) - 1ull;
    Tail t;
    for (int pb = 0; pb < total; pb += kP) {
        DMARK(10);
        ((volatile LDSA uint16_t*)mark)[lane] = 0xffffu;
        wave_lds_fence();
        const bool mine = kmem && excl >= pb && excl < pb + kP;
        mark[mine ? excl - pb : kP + lane] = (uint8_t)lane;
        wave_lds_fence();
        const uint32_t mm = ((volatile LDSA uint16_t*)mark)[lane];
        const uint32_t m0 = mm & 0xffu, m1 = mm >> 8;
        // owner of the lane's first byte: its own mark, else the last mark of an earlier lane
        const uint64_t lt_ = ballot(mm != 0xffffu) & below;
        const int js = lt_ ? 63 - __builtin_clzll(lt_) : lane;
        const uint32_t mj = lane_gather(mm, js);
        const int prevk = lt_ ? (int)((mj >> 8) != 0xffu ? (mj >> 8) : (mj & 0xffu)) : carry;
        const int k0 = m0 != 0xffu ? (int)m0 : prevk;
        const int k1 = m1 != 0xffu ? (int)m1 : k0;
        carry = rdlanei(k1, 63);
        const int le0 = (int)lane_gather((uint32_t)m_lend, k0), ls0 = (int)lane_gather((uint32_t)m_lsb, k0),
                  ms0 = (int)lane_gather((uint32_t)m_msrc, k0), of0 = (int)lane_gather((uint32_t)off, k0);
        int le1 = le0, ls1 = ls0, ms1 = ms0, of1 = of0;
        DST(2, 1);
        if (ballot(k1 != k0)) {
            DST(3, 1);
            le1 = (int)lane_gather((uint32_t)m_lend, k1);
            ls1 = (int)lane_gather((uint32_t)m_lsb, k1);
            ms1 = (int)lane_gather((uint32_t)m_msrc, k1);
            of1 = (int)lane_gather((uint32_t)off, k1);
        }
        DMARK(11);
        const int pbase = op + pb;
        const int thr = pbase + kP - SinkType::kWin;               // sources below: overwritten in the window
        const int ob0 = pb + 2 * lane, ob1 = ob0 + 1;
        int src0, src1;
        uint64_t done0, done1, far0, far1;
        const uint32_t v0 = owned_byte(w, O, op, pbase, thr, ob0, total, le0, ls0, ms0, of0, src0, done0, far0);
        const uint32_t v1 = owned_byte(w, O, op, pbase, thr, ob1, total, le1, ls1, ms1, of1, src1, done1, far1);
        DMARK(12);
        t.g0 = t.g1 = 0;
        const bool anyfar = (far0 | far1) != 0;
        if (anyfar) {   // far sources were flushed long ago: their stores must be done
            DST(5, 1);
            wait_vm();
            t.g0 = O.out.b_sc1(lane_on(far0) ? src0 : 0);
            t.g1 = O.out.b_sc1(lane_on(far1) ? src1 : 0);
        }
        t.far0 = far0; t.far1 = far1; t.done0 = done0; t.done1 = done1;
        t.v0 = v0; t.v1 = v1; t.src0 = src0; t.src1 = src1; t.ob0 = ob0; t.ob1 = ob1;
        t.pbase = pbase; t.op = op; t.total = total;
        DMARK(13);
        pass_tail(O, t, lane);
        DMARK(14);
    }
}

}  // namespace groups
