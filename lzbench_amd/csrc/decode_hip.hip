// lzbench_amd/csrc/decode_hip.hip -- LZ4 and snappy block decoders for gfx950.
//
// One 64-lane wavefront per chunk.  The compressed stream is read from a 512-byte register
// window (two VGPRs across the wave: v_readlane / ds_bpermute, no memory round trip); the
// last 4 KiB of decoded output stay in an LDS window (match sources there are LDS-to-LDS
// copies) and leave for HBM as aligned dword stores; far match sources are read back from the
// already-flushed output with L1-bypassing loads.  Sequences / tags are decoded a group at a
// time (groups::), with a checked one-at-a-time path for everything a group does not take.
//
// Acceptance rules follow the reference decoders so malformed input is rejected:
//   LZ4_decompress_safe   /root/reference/lz4/lz4.c:1707-1729, :1929-2151, :2170-2176
//   snappy RawUncompress  /root/reference/snappy/snappy.cc:819-1036, :1319-1407
// (lzbench itself calls LZ4_decompress_fast, compressors.cpp:358-362, which trusts its
// input; on valid streams both produce identical bytes.)
//
// Also here: the split zstd decoder (zsplit), the uniform zstd kernels, all launchers and debug hooks.  The windows
// and the group emitter are decode_win.h, the one-wave zstd decoder zstdd.h.  zstd_ragged_split_hip.hip still includes
// this file as text, under LZH_DEVICE_FUNCTIONS_ONLY, for zsplit's device functions alone.
#ifndef LZH_DEVICE_FUNCTIONS_ONLY
#define LZH_HDR_VAR   // (the tables external, as they were when zstdd stood here: profiles/decode_headers/README.md)
#endif
#include "decode_win.h"

// ---------------------------------------------------------------------------------------
// One LZ4 sequence at a time with every acceptance rule of LZ4_decompress_safe (lz4.c:1707-1729,
// :1929-2151): the path for what a group does not take (255-run lengths, the last-literals
// sequence, malformed input).  Returns 0 = continue, 1 = done (last literals), < 0 = error.
namespace checked {

using owin::kW;

template <class SinkType>
__device__ __forceinline__ int lz4_one(const Bytes& in, int cs, SinkType& O, Win& w, int cap, int& ip, int& op,
                                       int lane, int prefix = 0) {
    if (ip >= cs) return -ip - 1;
    w.ensure(ip, lane);
    const uint32_t tok = w.byte(ip++);
    int lit = (int)(tok >> 4);
    if (lit == 15) {
        if (ip >= cs - 15) return -ip - 1;
        for (int it = 0; it <= cs; it++) {
            w.ensure(ip, lane);
            const uint32_t s = w.byte(ip++);
            lit += (int)s;
            if (ip >= cs - 15 || s != 255) break;
        }
    }
    if (op + lit > cap - 12 || ip + lit > cs - 8) {
        if (ip + lit != cs || op + lit > cap) return -ip - 1;
        O.literals(w, in, ip, op, lit, lane);
        op += lit;
        return 1;
    }
    O.literals(w, in, ip, op, lit, lane);
    ip += lit;
    op += lit;
    w.ensure(ip, lane);
    const int off = (int)(w.byte(ip) | (w.byte(ip + 1) << 8));
    ip += 2;
    int ml = (int)(tok & 15u);
    if (ml == 15) {
        for (int it = 0; it <= cs; it++) {
            w.ensure(ip, lane);
            const uint32_t s = w.byte(ip++);
            ml += (int)s;
            if (ip >= cs - 4) return -ip - 1;
            if (s != 255) break;
        }
    }
    ml += 4;
    if (off > op + prefix) return -ip - 1;   // (prefix: earlier output of a linked frame, lz4.c:2404-2416)
    if (op + ml > cap - 5) return -ip - 1;
    if (off == 0) {
        for (int base = 0; base < ml; base += LZH_WAVE) {
            if (base + lane < ml) O.put(op + base + lane, 0);
            O.maybe_flush(op + min(base + LZH_WAVE, ml), lane);
        }
    } else {
        O.match(op, off, ml, lane);
    }
    op += ml;
    return 0;
}

}  // namespace checked

// ---------------------------------------------------------------------------------------
// Groups resolved lane-parallel.  Every lane parses "a sequence at ip + lane" in full (token, one
// literal-length byte, offset, one match-length byte) from the register window; binary lifting
// over the per-lane next-token links (chain_members) picks the real chain;
// the reference acceptance rules are checked per member lane against a DPP prefix sum of the
// output lengths, and the chain is cut before the first member that fails them (it, the last
// sequence and sequences with 255-run lengths go through the checked path).  Output bytes are
// assembled one per lane per pass: the owning sequence is found from per-pass start marks in
// LDS, literal bytes come from the register window, match bytes from the LDS output window (or
// global memory for far sources) in dependency rounds.
namespace groups {

using owin::kW;

// Lanes on the chain that starts at lane 0 and follows `link` (next lane, strictly increasing;
// >= 64 = leaves the group, 255 = the lane itself is not taken), by binary lifting: jump tables
// J_k = link^(2^k) through ds_bpermute, then every lane lifts from lane 0 to the furthest chain
// lane <= itself.  No scalar walk (the decoder is scalar-issue bound).
__device__ __forceinline__ uint64_t chain_members(int link, int lane) {
    // (every member takes >= 2 stream bytes -- a snappy literal tag + 1 byte or a COPY_1, LZ4 >= 3 --
    // so a chain from lane 0 has at most 32 members: jumps of 1..16 reach every one of them)
    const int J0 = min(link, LZH_WAVE);
    const int J1 = J0 < LZH_WAVE ? (int)lane_gather((uint32_t)J0, J0) : LZH_WAVE;
    const int J2 = J1 < LZH_WAVE ? (int)lane_gather((uint32_t)J1, J1) : LZH_WAVE;
    const int J3 = J2 < LZH_WAVE ? (int)lane_gather((uint32_t)J2, J2) : LZH_WAVE;
    const int J4 = J3 < LZH_WAVE ? (int)lane_gather((uint32_t)J3, J3) : LZH_WAVE;
    int x = 0, y;
    y = (int)lane_gather((uint32_t)J4, x); x = y <= lane ? y : x;
    y = (int)lane_gather((uint32_t)J3, x); x = y <= lane ? y : x;
    y = (int)lane_gather((uint32_t)J2, x); x = y <= lane ? y : x;
    y = (int)lane_gather((uint32_t)J1, x); x = y <= lane ? y : x;
    y = (int)lane_gather((uint32_t)J0, x); x = y <= lane ? y : x;
    return ballot(x == lane) & ballot(link != 255);   // (single compares: no VGPR round trip)
}

template <class SinkType>
__device__ int lz4_decode(const Bytes& in, int cs, SinkType& O, LDSA uint8_t* mark, LDSA uint8_t* ring, int cap,
                          int lane, int prefix = 0) {
    if (cap == 0) return (cs == 1 && in.b(0) == 0) ? 0 : -1;
    if (cs <= 0) return -1;
    Win w;
    w.bind(in, ring);
    w.load(0, lane);
    int ip = 0, op = 0;
    for (int guard = 0; guard <= cs; guard++) {
        DCLK(t0);
        DMARK(0);
        ip = unii(ip); op = unii(op);
        O.flushed = unii(O.flushed); O.ringlo = unii(O.ringlo);
        if (!w.covers(ip, ip + 2 * LZH_WAVE)) w.load(ip, lane);
        // ---- every lane parses a whole sequence at x = ip + lane (lz4.c:1707-1729, :1929-2151)
        const int x = ip + lane;
        const uint32_t tw = w.lane_word(x);
        const int ln = (int)((tw >> 4) & 15u), mc = (int)(tw & 15u), b1 = (int)((tw >> 8) & 255u);
        const int lit = ln == 15 ? 15 + b1 : ln;
        const int p1 = x + 1 + (ln == 15 ? 1 : 0);                // first literal byte
        const int po = p1 + lit;                                    // offset bytes
        const bool inwin = w.covers(po, po + 4);
        const uint32_t ow = w.lane_word(inwin ? po : x);
        const int off = (int)(ow & 0xffffu), b2 = (int)((ow >> 16) & 255u);
        const int ml = mc == 15 ? 19 + b2 : mc + 4;
        const int pe = po + 2 + (mc == 15 ? 1 : 0);                 // next token
        const bool cplx = !inwin || (ln == 15 && b1 == 255) || (mc == 15 && b2 == 255);
        const int link = cplx ? 255 : pe - ip;
        // ---- the real chain from lane 0
        DMARK(1);
        const uint64_t M = chain_members(link, lane);
        DMARK(2);
        // ---- acceptance rules per member (as lz4_one); the chain ends before the first failure
        const bool mem = lane_on(M);
        const int L = mem ? lit + ml : 0;
        const int incl = wave_incl_scan(L);
        const int excl = incl - L;
        const int opm = op + excl + lit;
        // (the failing members as a mask of single-compare ballots: a ballot of the compound bool goes through a VGPR)
        const uint64_t badm = M & (ballot(x >= cs) | (ballot(ln == 15) & ballot(x + 1 >= cs - 15)) | ballot(opm > cap - 12) |
                                   ballot(p1 + lit > cs - 8) | (ballot(mc == 15) & ballot(po + 3 >= cs - 4)) |
                                   ballot(off == 0) | ballot(off > opm + prefix) | ballot(opm + ml > cap - 5));
        const uint64_t keep = badm ? (M & ((1ull << __builtin_ctzll(badm)) - 1ull)) : M;
        if (!keep) {
            const int r = checked::lz4_one(in, cs, O, w, cap, ip, op, lane, prefix);
            DST(6, 1);
#if LZH_DEC_STATS
            DST(10, __builtin_amdgcn_s_memtime() - t0);
#endif
            if (r < 0) return r;
            if (r == 1) break;
            continue;
        }
        const int lastk = 63 - __builtin_clzll(keep);
        const int total = rdlanei(incl, lastk);
        const int ip_next = ip + rdlanei(pe - ip, lastk);
        DCLK(t1);
        DMARK(3);
        emit_group(w, O, mark, ip, op, total, keep, excl, (uint32_t)lit | ((uint32_t)ml << 16), (uint32_t)(p1 - ip),
                   off, lane);
#if LZH_DEC_STATS
        DCLK(t2);
        DST(0, 1);
        DST(1, __builtin_popcountll(keep));
        DST(7, total);
        DST(8, t1 - t0);
        DST(9, t2 - t1);
#endif
        op += total;
        ip = ip_next;
    }
    return op;
}


// snappy tags a group at a time (same scheme): every lane parses a tag at ip + lane (literal with
// at most one length byte, COPY_1/2/4), the walk follows the next-tag links, the acceptance rules
// of snappy_decode below (snappy.cc:848-952) are checked per member against the prefix sum, and
// the group is cut before the first failure (which, like 2..4-byte literal lengths, runs through
// the checked per-tag path).
// (nohdr: a fragment of a stream -- its tags without the varint, decoding exactly cap bytes; see
// lzh_snappy_split_kernel)
template <class SinkType>
__device__ int snappy_decode(const Bytes& in, int cs, SinkType& O, LDSA uint8_t* mark, LDSA uint8_t* ring, int cap,
                             int lane, bool nohdr = false) {
    Win w;
    w.bind(in, ring);
    w.load(0, lane);
    int ip = 0;
    uint32_t ulen = nohdr ? (uint32_t)cap : 0u;
    for (int shift = 0; !nohdr; shift += 7) {
        if (ip >= cs || shift >= 32) return -1;
        const uint32_t c = w.byte(ip++);
        const uint32_t val = c & 0x7fu;
        if (shift == 28 && val > 15) return -1;
        ulen |= val << shift;
        if (c < 128) break;
    }
    if (ulen > (uint32_t)cap) return -1;
    const int ul = (int)ulen;
    int op = 0;
    for (int guard = 0; guard <= cs && ip < cs; guard++) {
        ip = unii(ip); op = unii(op);
        O.flushed = unii(O.flushed); O.ringlo = unii(O.ringlo);
        if (!w.covers(ip, ip + 2 * LZH_WAVE)) w.load(ip, lane);
        const int x = ip + lane;
        const uint32_t tw = w.lane_word(x);
        const uint32_t c = tw & 0xffu, kind = c & 3u;
        int len, lit, nx, off = 0, p1 = x + 1;
        bool cplx = false, okr = true;
        if (kind == 0) {
            const int l6 = (int)(c >> 2) + 1;
            const bool one = l6 == 61;                              // one length byte
            cplx = l6 > 61;
            len = one ? (int)((tw >> 8) & 0xffu) + 1 : l6;
            p1 = x + 1 + (one ? 1 : 0);
            lit = len;
            nx = p1 + len;
            okr = (!one || x + 2 <= cs) && p1 + len <= cs;
        } else {
            const int extra = kind == 1 ? 1 : (kind == 2 ? 2 : 4);
            const uint32_t tw2 = w.lane_word(x + 1);
            if (kind == 1) {
                len = (int)((c >> 2) & 7u) + 4;
                off = (int)(((c >> 5) << 8) | ((tw >> 8) & 0xffu));
            } else {
                len = (int)(c >> 2) + 1;
                off = kind == 2 ? (int)((tw >> 8) & 0xffffu) : (int)tw2;
            }
            lit = 0;
            nx = x + 1 + extra;
            okr = nx <= cs && off > 0 && (uint32_t)off <= (uint32_t)cap;
        }
        const bool inwin = w.covers(x, nx + 4);
        // link: next tag lane; 255 = not parsed here; 254 = the stream ends after this tag
        const int link = (cplx || !inwin || x >= cs) ? 255 : (nx >= cs ? 254 : nx - ip);
        const uint64_t M = chain_members(link, lane);
        const bool mem = lane_on(M);
        const int L = mem ? len : 0;
        const int incl = wave_incl_scan(L);
        const int excl = incl - L;
        const int opm = op + excl;
        const uint64_t badm = M & (ballot(x >= cs) | ~ballot(okr) | ballot(opm + len > ul) |
                                   (ballot(kind != 0) & ballot(off > opm)));   // (single-compare ballots)
        const uint64_t keep = badm ? (M & ((1ull << __builtin_ctzll(badm)) - 1ull)) : M;
        if (!keep) {
            // one tag through the checked path (snappy.cc:848-952 rules)
            const uint32_t cc = w.byte(ip++);
            const uint32_t kk = cc & 3u;
            if (kk == 0) {
                int ln = (int)(cc >> 2) + 1;
                if (ln > 60) {
                    const int nb = ln - 60;
                    if (ip + nb > cs) return -1;
                    uint32_t v = 0;
                    for (int i = 0; i < nb; i++) v |= w.byte(ip + i) << (8 * i);
                    ln = (int)v + 1;
                    if (v >= 0x7fffffffu) return -1;
                    ip += nb;
                }
                if ((int64_t)ip + ln > cs || (int64_t)op + ln > ul) return -1;
                O.literals(w, in, ip, op, ln, lane);
                ip += ln;
                op += ln;
            } else {
                const int extra = kk == 1 ? 1 : (kk == 2 ? 2 : 4);
                if (ip + extra > cs) return -1;
                int ln;
                uint32_t of;
                if (kk == 1) {
                    ln = (int)((cc >> 2) & 7u) + 4;
                    of = ((cc >> 5) << 8) | w.byte(ip);
                } else {
                    ln = (int)(cc >> 2) + 1;
                    of = 0;
                    for (int i = 0; i < extra; i++) of |= w.byte(ip + i) << (8 * i);
                }
                ip += extra;
                if (of == 0 || of > (uint32_t)op || op + ln > ul) return -1;
                O.match(op, (int)of, ln, lane);
                op += ln;
            }
            continue;
        }
        const int lastk = 63 - __builtin_clzll(keep);
        const int total = rdlanei(incl, lastk);
        const int ip_next = ip + rdlanei(nx - ip, lastk);
        emit_group(w, O, mark, ip, op, total, keep, excl, (uint32_t)lit | ((uint32_t)(len - lit) << 16),
                   (uint32_t)(p1 - ip), off, lane);
        op += total;
        ip = ip_next;
    }
    return op == ul ? op : -1;
}

}  // namespace groups

// One chunk (or framed block) per wave; KW = bytes of the LDS output window.  The window sets the
// share of match sources read from the LDS instead of the flushed output in global memory, and the
// LDS per wave (hence waves per CU): lzh_launch_decompress picks the largest window whose occupancy
// still holds every chunk of the launch at once.
template <int KW>
__device__ __forceinline__ void decompress_chunk(LDSA uint8_t* win, int codec, const uint8_t* packed,
                                                 uint64_t packed_readable, const uint64_t* offsets,
                                                 const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size,
                                                 uint8_t* out, int32_t* status, uint32_t chunk0, const uint32_t* desc) {
    const int lane = threadIdx.x;
    const uint64_t chunk = (uint64_t)blockIdx.x + chunk0;
    uint64_t ooff, ioff;
    int part, cs;
    bool raw, nohdr = false;
    if (desc) {   // framed layouts: one 32-byte block descriptor each (frame_hip.hip FrameDesc)
        const uint32_t* d = desc + 8 * chunk;
        ioff = (uint64_t)uni(d[1]) << 32 | uni(d[0]);
        ooff = (uint64_t)uni(d[3]) << 32 | uni(d[2]);
        cs = (int)uni(d[4]);
        part = (int)uni(d[5]);
        const uint32_t fl = uni(d[6]);
        raw = (fl & 1u) != 0;
        nohdr = (fl & 8u) != 0;                 // a snappy fragment (lzh_snappy_split_kernel)
        if (fl & 22u) return;                   // a linked frame's block: lzh_decompress_linked_kernel; 16: skip
        if (part == 0) { if (lane == 0) status[chunk] = 0; return; }   // unused slot
    } else {
        ooff = chunk * chunk_size;
        if (ooff >= n_total) return;
        part = (int)min(chunk_size, n_total - ooff);
        ioff = offsets[chunk];
        cs = (int)csizes[chunk];
        raw = cs == part || codec == 2;
    }
#if LZH_DEC_STATS
    if (lane < 16) g_dst[lane] = 0;
    DCLK(tk0);
#endif
    const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, (uint64_t)cs + 16) : 0;
    Bytes rin, rout;
    rin.init(packed + ioff, readable);
    rout.init(out + ooff, (uint64_t)part);
    int r;
    if (raw) {
        copy_raw(rin, rout, part, lane);
        r = part;
    } else {
        owin::SinkT<KW> O{win, rout, 0, 0};
        LDSA uint8_t* mark = win + KW;
        LDSA uint8_t* ring = mark + 3 * LZH_WAVE;
        r = codec == 0 ? groups::lz4_decode(rin, cs, O, mark, ring, part, lane)
                       : groups::snappy_decode(rin, cs, O, mark, ring, part, lane, nohdr);
        if (r > 0) O.flush(r, lane);
    }
    if (lane == 0) status[chunk] = r;
#if LZH_DEC_STATS
    DST(11, 1);
    DST(12, __builtin_amdgcn_s_memtime() - tk0);
    if (lane < 16) atomicAdd(&lzh_dec_stats_buf[lane], g_dst[lane]);
#endif
}

#ifndef LZH_DEVICE_FUNCTIONS_ONLY   // (zstd_ragged_split_hip.hip includes this file for its device functions alone)
// output window | start marks | input ring
#define LZH_DEC_KERNEL(NAME, KW)                                                                            \
    extern "C" __global__ void __launch_bounds__(64)                                                       \
    NAME(int codec, const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,              \
         const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size, uint8_t* out, int32_t* status,     \
         uint32_t chunk0, const uint32_t* desc) {                                                          \
        __shared__ __attribute__((aligned(16))) uint8_t win[KW + 3 * LZH_WAVE + kRingBytes];              \
        decompress_chunk<KW>((LDSA uint8_t*)win, codec, packed, packed_readable, offsets, csizes, n_total,  \
                             chunk_size, out, status, chunk0, desc);                                       \
    }
LZH_DEC_KERNEL(lzh_decompress_v2_kernel, owin::kW)
LZH_DEC_KERNEL(lzh_decompress_w8k_kernel, 8192)
LZH_DEC_KERNEL(lzh_decompress_w16k_kernel, 16384)
#undef LZH_DEC_KERNEL

// LZ4 frames with linked blocks (frame_hip.hip marks their descriptors: flags 2 = a frame's first
// block, pad = its block count; 4 = a later block): one wave per frame decodes the blocks in order,
// each with the frame's output before it as its prefix (LZ4F_updateDict's prefix mode,
// lz4frame.c:1290-1306; LZ4_decompress_safe_usingDict, lz4.c:2404-2416): a match may reach back
// into earlier blocks (read from global memory, the window starts empty per block), and the offset
// check fails only past the frame's start.  Waves of other descriptors exit at once.
extern "C" __global__ void __launch_bounds__(64)
lzh_decompress_linked_kernel(const uint8_t* packed, uint64_t packed_readable, uint8_t* out, int32_t* status,
                             const uint32_t* desc) {
    __shared__ __attribute__((aligned(16))) uint8_t win[owin::kW + 3 * LZH_WAVE + kRingBytes];
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint32_t* d0 = desc + 8 * chunk;
    if (!(uni(d0[6]) & 2u)) return;
    const uint32_t nlink = uni(d0[7]);
    const uint64_t foff = (uint64_t)uni(d0[3]) << 32 | uni(d0[2]);   // the frame's output start
    for (uint32_t bi = 0; bi < nlink; bi++) {
        const uint32_t* d = desc + 8 * (chunk + bi);
        const uint64_t ioff = (uint64_t)uni(d[1]) << 32 | uni(d[0]);
        const uint64_t ooff = (uint64_t)uni(d[3]) << 32 | uni(d[2]);
        const int cs = (int)uni(d[4]), part = (int)uni(d[5]);
        const bool raw = (uni(d[6]) & 1u) != 0;
        wait_vm();   // (the previous block's output stores are done before its bytes are read back)
        const int prefix = (int)(ooff - foff);
        const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, (uint64_t)cs + 16) : 0;
        Bytes rin, rout;
        rin.init(packed + ioff, readable);
        rout.init(out + foff, (uint64_t)prefix + part);
        rout.sh += prefix;                    // (block positions; earlier output at negative ones)
        int r;
        if (raw) {
            copy_raw(rin, rout, part, lane);
            r = part;
        } else {
            owin::Sink O{(LDSA uint8_t*)win, rout, 0, 0};
            LDSA uint8_t* mark = (LDSA uint8_t*)win + owin::kW;
            LDSA uint8_t* ring = mark + 3 * LZH_WAVE;
            r = groups::lz4_decode(rin, cs, O, mark, ring, part, lane, prefix);
            if (r > 0) O.flush(r, lane);
        }
        if (lane == 0) status[chunk + bi] = r;
        if (r < 0) {   // the frame is bad: its remaining blocks are not decoded
            for (uint32_t bj = bi + 1 + (uint32_t)lane; bj < nlink; bj += LZH_WAVE) status[chunk + bj] = -1;
            break;
        }
    }
}
#endif

// ---------------------------------------------------------------------------------------
// Snappy chunks of more than one 64 KiB fragment, decoded a fragment per wave.  The reference
// compressor compresses every 64 KiB fragment of its input on its own (snappy.cc:1042-1072: a fresh
// table per fragment, candidates only inside it), so the tags of a stream it wrote start anew at every
// multiple of 64 KiB of output and no copy reaches into an earlier fragment.  lzh_snappy_split_kernel
// walks a chunk's tags (one wave per chunk: every lane parses the tag at ip + lane, a scalar walk
// follows the next-tag links and sums the output lengths) and records the tag that starts each
// fragment; the fragments then decode in parallel as headerless streams of exactly their size
// (descriptor flag 8).  A chunk that the walk does not split cleanly (a tag across a fragment start, a
// varint that is not the chunk's size, a stored chunk, a walk off the stream) or any fragment of which
// fails (a copy into an earlier fragment is valid snappy, just not what the reference writes) is
// decoded whole by the serial decoder afterwards, so every verdict and every byte of such a chunk is
// the serial decoder's.  An accepted split decodes the same tags in the same order as the serial
// decoder: the fragments partition the chunk's tag sequence, each ends exactly at its share of the
// stream and of the output, and a copy accepted inside a fragment is accepted in the chunk.
namespace snsplit {
constexpr int kFragLog = 16;
constexpr uint32_t kMaxFrags = 64;   // chunks of up to 4 MiB (larger ones decode whole)
constexpr uint32_t kMinFrags = 8;    // (by default; see lzh_snappy_split_temp)
__host__ __device__ inline uint32_t frags(uint64_t chunk_size) { return (uint32_t)((chunk_size + 65535) >> kFragLog); }
}

#ifndef LZH_DEVICE_FUNCTIONS_ONLY
extern "C" __global__ void __launch_bounds__(64)
lzh_snappy_split_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                        const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size, uint32_t F, uint32_t* desc,
                        uint32_t* cflag) {
    using namespace snsplit;
    __shared__ __attribute__((aligned(16))) uint8_t ring[kRingBytes];
    __shared__ uint32_t bnd[kMaxFrags + 1];
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint64_t ooff = chunk * chunk_size;
    if (ooff >= n_total) return;
    const int part = (int)min(chunk_size, n_total - ooff);
    const uint64_t ioff = offsets[chunk];
    const int cs = (int)csizes[chunk];
    const int nf = (part + (1 << kFragLog) - 1) >> kFragLog;
    bool ok = cs != part && nf > 1 && nf <= (int)F && F <= kMaxFrags;
    int ip = 0, op = 0, nb = 0;
    if (ok) {   // (a uniform walk: ip, op, nb in scalar registers)
        const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, (uint64_t)cs + 16) : 0;
        Bytes rin;
        rin.init(packed + ioff, readable);
        Win w;
        w.bind(rin, (LDSA uint8_t*)ring);
        w.load(0, lane);
        uint32_t ulen = 0;
        for (int shift = 0;; shift += 7) {   // varint32 uncompressed length (snappy.cc:1319-1331)
            if (ip >= cs || shift >= 32) { ok = false; break; }
            const uint32_t c = w.byte(ip++);
            ulen |= (c & 0x7fu) << shift;
            if (c < 128) break;
        }
        ok = ok && ulen == (uint32_t)part;
        if (lane == 0) bnd[0] = (uint32_t)ip;   // fragment 0 starts after the varint
        nb = 1;
        for (int guard = 0; ok && ip < cs && guard <= cs; guard++) {
            ip = unii(ip); op = unii(op); nb = unii(nb);
            if (!w.covers(ip, ip + 2 * LZH_WAVE)) w.load(ip, lane);
            // the tag at x = ip + lane: its stream length and output length (snappy.cc:848-952)
            const int x = ip + lane;
            const uint32_t tw = w.lane_word(x);
            const uint32_t c = tw & 0xffu, kind = c & 3u;
            uint32_t tw2 = 0;                       // (a 4-byte literal length reaches byte x + 4)
            if (ballot(c == 0xfcu)) tw2 = w.lane_word(x + 1);
            uint32_t len, sl;                       // output bytes, stream bytes after the tag byte
            if (kind == 0) {
                const uint32_t l6 = (c >> 2) + 1u;
                const uint32_t eb = l6 > 60u ? l6 - 60u : 0u;   // 1..4 length bytes
                const uint32_t v = eb == 4u ? tw2 : ((tw >> 8) & ((1u << (8u * eb)) - 1u));
                const uint32_t l = eb ? (v >= 0x00ffffffu ? 0x00ffffffu : v + 1u) : l6;   // (beyond any chunk)
                len = l;
                sl = eb + l;
            } else {
                len = kind == 1 ? ((c >> 2) & 7u) + 4u : (c >> 2) + 1u;
                sl = kind == 1 ? 1u : (kind == 2 ? 2u : 4u);
            }
            const int adv_l = lane + 1 + (int)sl;              // next tag, from ip (> lane)
            // the chain from lane 0 (binary lifting, as the decoder's groups); lanes at or past the
            // stream's end are not tags
            // (255 is chain_members' "not a tag": a real link that leaves the window is any value >= 64)
            const int link = x >= cs ? 255 : min(adv_l, 254);
            const uint64_t M = groups::chain_members(link, lane);
            const bool mem = lane_on(M);
            const int L = mem ? (int)len : 0;
            const int incl = groups::wave_incl_scan(L);
            const int start = op + incl - L;                   // a member's first output byte
            // a member starting on a multiple of 64 KiB starts that fragment
            const bool fb = mem && start > 0 && (start & ((1 << kFragLog) - 1)) == 0 && (start >> kFragLog) < nf;
            if (fb) bnd[start >> kFragLog] = (uint32_t)x;
            nb += __builtin_popcountll(ballot(fb));
            const int lastk = 63 - __builtin_clzll(M | 1ull);
            op += rdlanei(incl, lastk);
            ip += rdlanei(adv_l, lastk);
            if (op > part) ok = false;
        }
        ok = ok && ip == cs && op == part && nb == nf;
    }
    wave_lds_fence();
    uint32_t* D = desc + chunk * (uint64_t)F * 8;
    for (int j = lane; j < (int)F; j += LZH_WAVE) {   // fragment j; unused slots decode nothing (ds = 0)
        uint32_t a = 0, e = 0, ds = 0;
        if (ok && j < nf) {
            a = bnd[j];
            e = j + 1 < nf ? bnd[j + 1] : (uint32_t)cs;
            ds = (uint32_t)min(1 << kFragLog, part - (j << kFragLog));
        }
        const uint64_t src = ioff + a, dst = ooff + ((uint64_t)j << kFragLog);
        uint32_t* d = D + 8 * j;
        d[0] = (uint32_t)src; d[1] = (uint32_t)(src >> 32);
        d[2] = (uint32_t)dst; d[3] = (uint32_t)(dst >> 32);
        d[4] = e - a; d[5] = ds; d[6] = 8u; d[7] = 0u;
    }
    if (lane == 0) cflag[chunk] = ok ? 0u : 1u;
}

// chunks finished by fragments since the last reset (tests: lzh_debug_snappy_split_done)
__device__ unsigned long long lzh_snsplit_done;

// per chunk: split and every fragment decoded exactly its size -> the chunk's status; else a whole-chunk
// descriptor for the serial pass (flag 16 = skip for the others)
extern "C" __global__ void __launch_bounds__(256)
lzh_snappy_join_kernel(const uint64_t* offsets, const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size,
                       uint32_t F, const uint32_t* desc, const int32_t* fstat, const uint32_t* cflag, uint32_t* sdesc,
                       int32_t* status, uint32_t nchunks) {
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (c >= nchunks) return;
    const uint64_t ooff = c * chunk_size;
    const uint32_t part = (uint32_t)min(chunk_size, n_total - ooff);
    bool whole = cflag[c] != 0u;
    for (uint32_t j = 0; !whole && j < F; j++) {
        const uint32_t ds = desc[(c * F + j) * 8 + 5];
        if (ds && fstat[c * F + j] != (int32_t)ds) whole = true;
    }
    uint32_t* S = sdesc + c * 8;
    if (whole) {
        const uint64_t io = offsets[c];
        const uint32_t cs = csizes[c];
        S[0] = (uint32_t)io; S[1] = (uint32_t)(io >> 32);
        S[2] = (uint32_t)ooff; S[3] = (uint32_t)(ooff >> 32);
        S[4] = cs; S[5] = part; S[6] = cs == part ? 1u : 0u; S[7] = 0u;
    } else {
        S[0] = S[1] = S[2] = S[3] = S[4] = S[5] = S[7] = 0u;
        S[6] = 16u;
        status[c] = (int32_t)part;
        atomicAdd(&lzh_snsplit_done, 1ull);
    }
}

#if LZH_DEC_STATS
extern "C" int lzh_debug_dec_stats(unsigned long long* host, int reset) {
    if (reset) {
        unsigned long long z[16] = {};
        return hipMemcpyToSymbol(HIP_SYMBOL(lzh_dec_stats_buf), z, sizeof(z)) == hipSuccess ? 0 : -1;
    }
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(lzh_dec_stats_buf), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
#endif   // LZH_DEVICE_FUNCTIONS_ONLY

#include "zstdd.h"   // (where namespace zstdd stood: the object registers its device variables in the order it did)
// ---------------------------------------------------------------------------------------
// zstd decoding in three kernels.  The sequence section's decoding chain (bit reader, three FSE
// states, repcodes: ZSTD_decodeSequence, zstd_decompress_block.c:1169-1270) is serial within a
// block but independent between frames, so it runs one frame per LANE; what surrounds it is
// wave-parallel per frame:
//  1. lzh_zstd_hdr_kernel (one wave per frame): frame header, block walk, literal sections (the
//     Huffman streams decode into the frame's output tail), sequence-section headers; the FSE
//     tables it builds go to global memory per block.  Everything that does not need the output
//     position is checked here, in decode_frame's order.
//  2. lzh_zstd_seq_kernel (kFPW frames per wave, one per lane, tables in LDS): the sequences, with
//     every check of ZSTD_execSequence that depends on the output position; writes (ll, ml, offset)
//     per sequence.
//  3. lzh_zstd_exec_kernel (one wave per frame): executes them 64 at a time (groups::emit_group),
//     raw / RLE blocks and the content checksum.
// A frame that does not fit the layout (more blocks than bmax, more sequences than smax, a length
// of 2^17 or more) is decoded by lzh_zstd_decompress_kernel (the one-wave-per-frame decoder above)
// after the three.  Verdicts equal decode_frame's: every check is made, on the same quantities;
// only the order between checks differs, and every one of them reports kErrCorrupt.
//
// Literals of every block whose literal section is not raw live at the frame's output tail,
// block after block: [n - L, n) for L literals in all, so that the output of an accepted frame
// never overtakes a literal not yet copied (it holds every literal, and matches only add bytes).
namespace zsplit {
using namespace zstdd;

constexpr int kFPW = 8;              // frames per sequence-decoding wave (lanes 0 .. kFPW-1)
// the dummy stores' area after the frames' temp (512 bytes a sequence wave: a wave's lanes without a record
// store into their own wave's slice -- one shared slice for every wave was an L2 hot spot)
inline __host__ __device__ uint64_t zdummy_bytes(uint64_t nchunks) {   // (two launches' worth: see the launcher)
    const uint64_t w = (nchunks + kFPW - 1) / kFPW;
    return 2 * 512 * (w ? w : 1);
}
// A block's sequence tables in global memory (kSlot bytes): LL u32[512] | ML u32[512] | OF u16[256].
// LL / ML cell: next-state base (9) | nbBits << 9 (4) | extra bits << 13 (5) | pow << 18 | lo << 19
// (7): the baseline is lo, or 2^extra + lo for the codes whose baseline is >= 128 (LL 2^n, ML
// 2^n + 3): no baseline table on the chain.  OF cell (16 bits): e | code << 9 with e = 2 * base +
// 2^nbBits (a next-state base is a multiple of 2^nbBits: nbBits = ctz(e)).
constexpr int kSlot = 4608;
constexpr int kGo = 0, kLegacy = 1, kDone = 2;
constexpr int kLenBits = 17;         // (ll, ml, offset) packed as 17 + 17 + 30 bits

struct ZBlk {                        // a block of the frame (header kernel)
    uint32_t type;                   // 0 raw, 1 RLE, 2 compressed
    uint32_t ltype;                  // literals section type (compressed blocks)
    uint32_t pos;                    // raw: data position in the frame; RLE: the byte; else sequence stream start
    uint32_t size;                   // raw / RLE: block size; else sequence stream bytes
    uint32_t rs;                     // literals
    uint32_t lit;                    // literals' position: ltype 0 in the frame, else in the output
    uint32_t nseq;
    uint32_t logs;                   // accuracy logs LL | OF << 8 | ML << 16
    uint32_t tll, tof, tml;          // the blocks (of this frame) whose table slots hold LL / OF / ML
    uint32_t pad;
};
// blocks, content size, checksum position (-1: none); sv: the sequence kernel's verdict (kGo, kLegacy or
// an error), applied by the execution kernel -- the sequence kernel runs beside the literal kernels, which
// write zst / status themselves, and their verdict comes first
struct ZFrame { int32_t nblk, n, ccrc, sv, nsq, pad0, pad1, pad2; };   // (nsq: the frame's sequences)
struct ZExe { uint32_t op0, seq0; };             // a block's output position and first sequence
// a Huffman-coded literal section (header kernel -> literal kernel): its frame, the block whose
// table slot holds its table, the table log, whether the reference would decode it with the
// double-symbol decoder, streams, output position, symbols per stream (the 4th: last), streams
constexpr int kHufSlot = 4096;                   // a table of up to 2^11 16-bit cells (symbol | nbBits << 8)
struct ZHuf {
    uint32_t frame, tblk, tl, x2, ns, dst, seg, last;
    uint32_t s0[4], sz[4];
};

struct ZLayout {
    uint64_t bmax, smax, stride;
    __host__ __device__ uint64_t exe() const { return bmax * sizeof(ZBlk); }
    __host__ __device__ uint64_t cells() const { return exe() + bmax * sizeof(ZExe); }
    __host__ __device__ uint64_t hufs() const { return cells() + bmax * kSlot; }
    __host__ __device__ uint64_t seqs() const { return hufs() + bmax * kHufSlot; }
};
__host__ __device__ inline ZLayout zlayout(uint64_t chunk) {
    ZLayout L;
    L.bmax = (chunk + kBlockMax - 1) / kBlockMax + 1;   // the compressor writes ceil(chunk / 128 KiB) blocks
    L.smax = chunk / 4 + 64;                            // (its matches are >= 4 bytes)
    L.stride = (L.seqs() + L.smax * 8 + 255) & ~255ull;
    return L;
}

// one compressed block's literal section and sequence-section header (decode_block up to the
// sequences); lacc = the next literal position at the output tail
__device__ __forceinline__ int hdr_block(const Bytes& rin, const Bytes& rout, ZWin& fw, LDSA Lds& L, FrameState& F,
                                         int bs, int be, int& lacc, ZBlk& B, uint8_t* cells, int b, int& tll, int& tof,
                                         int& tml, int& thuf, uint8_t* hufs, ZHuf* jobs, uint32_t* njobs, uint32_t frame,
                                         int lane) {
    const uint32_t b0 = fbyte(fw, bs, lane);
    const int ltype = (int)(b0 & 3u), sf = (int)((b0 >> 2) & 3u);
    int rs, seqpos;
    if (ltype <= 1) {
        int hsz;
        if ((sf & 1) == 0) { hsz = 1; rs = (int)(b0 >> 3); }
        else if (sf == 1) { hsz = 2; rs = (int)((b0 >> 4) + (fbyte(fw, bs + 1, lane) << 4)); }
        else { hsz = 3; rs = (int)((b0 >> 4) + (fbyte(fw, bs + 1, lane) << 4) + (fbyte(fw, bs + 2, lane) << 12)); }
        if (rs > kBlockMax) return ZC;
        if (ltype == 0) {
            if (bs + hsz + rs > be) return ZC;
            B.lit = (uint32_t)(bs + hsz);
            seqpos = bs + hsz + rs;
        } else {
            if (bs + hsz + 1 > be) return ZC;   // (rs > fcs - op: the sequence kernel)
            const uint32_t v = fbyte(fw, bs + hsz, lane);
            for (int i = lane; i < rs; i += LZH_WAVE) rout.st8(lacc + i, v);
            B.lit = (uint32_t)lacc;
            lacc += rs;
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
        if (rs > kBlockMax || bs + hsz + cs > be) return ZC;
        int p = bs + hsz;
        if (ltype == 2) {
            int tl = 0;
            ZCLK(F, 0);
            const int u = read_huf(fw, rin, p, bs + hsz + cs, L, tl, lane);
            ZCLK(F, 1);
            if (u < 0) return u;
            F.hufV = true;
            F.hufTl = tl;
            F.hufX2 = sf != 0 && huf_select_x2(rs, cs);
            p += u;
        } else if (!F.hufV) {
            return ZC;
        }
        if (rs == 0 && sf != 0 && ltype == 2) return ZC;
        if (F.hufTl > 11) return kLegacy;            // (the literal kernel's table slots hold 2^11 cells)
        if (ltype == 2) {                            // the table to the block's slot
            uint32_t* dst = (uint32_t*)(hufs + (size_t)b * kHufSlot);
            const LDSA uint32_t* src = (const LDSA uint32_t*)L.huf;
            for (int c = lane; c < (1 << F.hufTl) / 2; c += LZH_WAVE) dst[c] = src[c];
            thuf = b;
        }
        // the streams' geometry and end marks, as huf_streams checks them; the literal kernel decodes
        const int csize = bs + hsz + cs - p, ns = sf == 0 ? 1 : 4;
        ZHuf J{};
        J.frame = frame;
        J.tblk = (uint32_t)thuf;
        J.tl = (uint32_t)F.hufTl;
        J.x2 = F.hufX2 ? 1u : 0u;
        J.ns = (uint32_t)ns;
        J.dst = (uint32_t)lacc;
        if (ns == 4) {
            if (csize < 10) return ZC;
            const int z1 = (int)(fword(fw, p, lane) & 0xffffu), z2 = (int)(fword(fw, p + 2, lane) & 0xffffu),
                      z3 = (int)(fword(fw, p + 4, lane) & 0xffffu);
            const int z4 = csize - 6 - z1 - z2 - z3;
            if (z4 < 1) return ZC;
            const int seg = (rs + 3) / 4, last = rs - 3 * seg;
            if (last < 0) return ZC;
            if (z1 <= 0 || z2 <= 0 || z3 <= 0) return ZC;
            J.seg = (uint32_t)seg;
            J.last = (uint32_t)last;
            const int p1 = p + 6;
            J.s0[0] = (uint32_t)p1; J.s0[1] = (uint32_t)(p1 + z1); J.s0[2] = (uint32_t)(p1 + z1 + z2);
            J.s0[3] = (uint32_t)(p1 + z1 + z2 + z3);
            J.sz[0] = (uint32_t)z1; J.sz[1] = (uint32_t)z2; J.sz[2] = (uint32_t)z3; J.sz[3] = (uint32_t)z4;
        } else {
            if (csize <= 0) return ZC;
            J.seg = J.last = (uint32_t)rs;
            J.s0[0] = (uint32_t)p;
            J.sz[0] = (uint32_t)csize;
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < ns && fbyte(fw, (int)(J.s0[k] + J.sz[k]) - 1, lane) == 0) return ZC;   // (BIT_initDStream: no end mark)
        if (lane == 0) jobs[atomicAdd(njobs, 1u)] = J;
        B.lit = (uint32_t)lacc;
        lacc += rs;
        seqpos = bs + hsz + cs;
    }
    B.ltype = (uint32_t)ltype;
    B.rs = (uint32_t)rs;
    // sequences section header (ZSTD_decodeSeqHeaders)
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
    B.nseq = (uint32_t)nseq;
    if (nseq > 0) {
        if (p >= be) return ZC;
        const uint32_t modes = fbyte(fw, p++, lane);
        if (modes & 3u) return ZC;
        // a table built in this block goes to the block's slot; "repeat" keeps the previous slot
        auto table = [&](int mode, int which, LDSA Cell* T, int& al, bool& valid, int& slot) -> bool {
            const int u = seq_table(fw, p, be, mode, which, T, al, valid, L, lane);
            if (u < 0) return false;
            p += u;
            if (mode != 3) {   // the cells in the sequence kernel's formats (kSlot)
                uint8_t* dst = cells + (size_t)b * kSlot;
                for (int c = lane; c < (1 << al); c += LZH_WAVE) {
                    const Cell e = T[c];
                    const uint32_t nx = c_next(e), nb = (uint32_t)c_nb(e), add = (uint32_t)c_add(e), sym = c_sym(e);
                    if (which == 1) {
                        ((uint16_t*)(dst + 4096))[c] = (uint16_t)((2u * nx + (1u << nb)) | (sym << 9));
                    } else {
                        const uint32_t base = which == 0 ? kLLBase[sym] : kMLBase[sym];
                        const uint32_t pw = base >= 128u;
                        const uint32_t lo = pw ? base - (1u << add) : base;
                        ((uint32_t*)(dst + (which == 0 ? 0 : 2048)))[c] = nx | (nb << 9) | (add << 13) | (pw << 18) | (lo << 19);
                    }
                }
                slot = b;
            }
            return true;
        };
        ZCLK(F, 0);
        if (!table((int)(modes >> 6), 0, L.ll, F.llA, F.llV, tll)) return ZC;
        if (!table((int)((modes >> 4) & 3u), 1, L.of, F.ofA, F.ofV, tof)) return ZC;
        if (!table((int)((modes >> 2) & 3u), 2, L.ml, F.mlA, F.mlV, tml)) return ZC;
        ZCLK(F, 3);
        B.logs = (uint32_t)F.llA | ((uint32_t)F.ofA << 8) | ((uint32_t)F.mlA << 16);
        B.tll = (uint32_t)tll; B.tof = (uint32_t)tof; B.tml = (uint32_t)tml;
        B.pos = (uint32_t)p;
        B.size = (uint32_t)(be - p);
    } else if (p != be) {
        return ZC;
    }
    return 0;
}

// the frame's header and blocks (decode_frame without the sequences); returns kGo / kLegacy or an error
__device__ __forceinline__ int hdr_frame_body(const Bytes& rin, const Bytes& rout, int cs, LDSA Lds& L, int cap,
                                              uint8_t* zb, const ZLayout& Z, ZFrame& fr, int lane, FrameState& F,
                                              ZHuf* jobs, uint32_t* njobs, uint32_t frame) {
    ZWin fw;
    fw.bind(rin, nullptr);
    fw.load(0, lane);
    if (cs < 9) return ZC;
    const uint32_t magic = fword(fw, 0, lane);
    if (magic != 0xFD2FB528u) return (magic & 0xFFFFFFF0u) == 0x184D2A50u ? kErrUnsupported : kErrCorrupt;
    const uint32_t fhd = fbyte(fw, 4, lane);
    const int fcsf = (int)(fhd >> 6), single = (int)((fhd >> 5) & 1u);
    if (fhd & 8u) return ZC;
    const int ccrc = (fhd & 4u) ? 4 : 0;
    int p = 5;
    if (!single) {
        const uint32_t wd = fbyte(fw, p++, lane);
        if ((wd >> 3) + 10 > 27) return kErrUnsupported;
    }
    const int dsz = (int)(fhd & 3u) == 3 ? 4 : (int)(fhd & 3u);
    uint32_t dict = 0;
    for (int i = 0; i < dsz; i++) dict |= fbyte(fw, p + i, lane) << (8 * i);
    p += dsz;
    if (dict) return kErrUnsupported;
    const int fsz = fcsf == 0 ? (single ? 1 : 0) : (fcsf == 1 ? 2 : (fcsf == 2 ? 4 : 8));
    if (fsz == 0) return kErrUnsupported;
    uint64_t fcs = 0;
    for (int i = 0; i < fsz; i++) fcs |= (uint64_t)fbyte(fw, p + i, lane) << (8 * i);
    if (fsz == 2) fcs += 256;
    p += fsz;
    if (fcs > (uint64_t)cap) return ZC;
    const int n = (int)fcs;
    // walk the block headers and literal-section sizes first: the tail layout needs the total
    int nb = 0, ltot = 0;
    {
        int q = p;
        for (int guard = 0; guard <= cs; guard++) {
            if (q + 3 > cs) return ZC;
            const uint32_t bh = fbyte(fw, q, lane) | (fbyte(fw, q + 1, lane) << 8) | (fbyte(fw, q + 2, lane) << 16);
            q += 3;
            const int last = (int)(bh & 1u), type = (int)((bh >> 1) & 3u), bsz = (int)(bh >> 3);
            if (bsz > kBlockMax) return ZC;
            if (++nb > (int)Z.bmax) return kLegacy;
            if (type == 0) {
                if (q + bsz > cs) return ZC;
                q += bsz;
            } else if (type == 1) {
                if (q + 1 > cs) return ZC;
                q += 1;
            } else if (type == 2) {
                if (q + bsz > cs || bsz < 1) return ZC;
                const uint32_t b0 = fbyte(fw, q, lane);
                const int ltype = (int)(b0 & 3u), sf = (int)((b0 >> 2) & 3u);
                int rs;
                if (ltype <= 1) {
                    const int hsz = (sf & 1) == 0 ? 1 : (sf == 1 ? 2 : 3);
                    if (q + hsz > cs) return ZC;
                    rs = (sf & 1) == 0 ? (int)(b0 >> 3)
                                       : (sf == 1 ? (int)((b0 >> 4) + (fbyte(fw, q + 1, lane) << 4))
                                                  : (int)((b0 >> 4) + (fbyte(fw, q + 1, lane) << 4) +
                                                          (fbyte(fw, q + 2, lane) << 12)));
                } else {
                    const int hsz = sf <= 1 ? 3 : (sf == 2 ? 4 : 5);
                    const int bits = sf <= 1 ? 10 : (sf == 2 ? 14 : 18);
                    if (hsz > bsz) return ZC;
                    uint64_t h = 0;
                    for (int i = 0; i < hsz; i++) h |= (uint64_t)fbyte(fw, q + i, lane) << (8 * i);
                    rs = (int)((h >> 4) & ((1u << bits) - 1));
                }
                if (rs > kBlockMax) return ZC;
                if (ltype != 0) ltot += rs;
                q += bsz;
            } else {
                return ZC;
            }
            if (last) break;
        }
    }
    if (ltot > n) return ZC;   // an accepted frame's output holds every literal
    ZBlk* blk = (ZBlk*)zb;
    uint8_t* cells = zb + Z.cells();
    int lacc = n - ltot, tll = 0, tof = 0, tml = 0, thuf = 0, nsq = 0;
    for (int b = 0; b < nb; b++) {
        const uint32_t bh = fbyte(fw, p, lane) | (fbyte(fw, p + 1, lane) << 8) | (fbyte(fw, p + 2, lane) << 16);
        p += 3;
        const int type = (int)((bh >> 1) & 3u), bsz = (int)(bh >> 3);
        ZBlk B{};
        B.type = (uint32_t)type;
        if (type == 0) {
            B.pos = (uint32_t)p;
            B.size = (uint32_t)bsz;
            p += bsz;
        } else if (type == 1) {
            B.pos = fbyte(fw, p, lane);
            B.size = (uint32_t)bsz;
            p += 1;
        } else {
            const int r = hdr_block(rin, rout, fw, L, F, p, p + bsz, lacc, B, cells, b, tll, tof, tml, thuf, zb + Z.hufs(),
                                    jobs, njobs, frame, lane);
            if (r != 0) return r;   // (an error, or kLegacy)
            p += bsz;
            nsq += (int)B.nseq;
        }
        if (lane == 0) blk[b] = B;
    }
    if (p + ccrc != cs) return ZC;
    fr.nsq = nsq;
    fr.nblk = nb;
    fr.n = n;
    fr.ccrc = ccrc ? p : -1;
    return kGo;
}

__device__ __forceinline__ int hdr_frame(const Bytes& rin, const Bytes& rout, int cs, LDSA Lds& L, int cap, uint8_t* zb,
                                         const ZLayout& Z, ZFrame& fr, int lane, unsigned long long* stats, ZHuf* jobs,
                                         uint32_t* njobs, uint32_t frame) {
    FrameState F{1, 4, 8, 0, 0, 0, false, false, false, false, false, 0, {0, 0, 0, 0, 0, 0, 0, 0}, 0};
    if (LZH_ZSTD_STATS) F.clk_last = __builtin_amdgcn_s_memtime();
    const int r = hdr_frame_body(rin, rout, cs, L, cap, zb, Z, fr, lane, F, jobs, njobs, frame);
    ZCLK(F, 7);
    if (LZH_ZSTD_STATS && stats && lane == 0)
        for (int i = 0; i < kZClk; i++) atomicAdd(&stats[i], (unsigned long long)F.clk[i]);
    return r;
}

// The sequence kernel's LDS (kFPW lanes; a "row" holds one dword per lane, as an LDS-DMA
// (global_load_lds_dword) writes it: lane i at row + 4 i): LL cells 512 rows, ML 512, OF 128 (two
// 16-bit cells a dword), the bit-stream ring (64 rows: stream dword d at row d mod 64, two halves of
// 32-dword blocks, + a mirror of row 0), the sequences buffered between flush points (kSB per lane,
// 8 bytes).  39 456 bytes: 4 waves per CU.
constexpr int kRow = 4 * kFPW;
constexpr int kSB = 16;                         // steps between flush / fill points
constexpr int kLdsML = 512 * kRow, kLdsOF = 1024 * kRow, kLdsRing = 1152 * kRow, kLdsSB = 1217 * kRow;
constexpr int kLdsSeq = kLdsSB;

__device__ __forceinline__ void dma_row(const uint8_t* src, LDSA uint8_t* row) {
    __builtin_amdgcn_global_load_lds((const void*)src, (LDSA void*)row, 4, 0, 0);
}
// s_waitcnt immediate for vmcnt(n) alone (gfx9: vmcnt bits [3:0] and [15:14], expcnt / lgkmcnt at max)
constexpr int vmcnt_imm(int n) { return 0x0F70 | (n & 15) | ((n >> 4) << 14); }
// one dword per lane from a buffer resource into an LDS row (out-of-range offsets read 0, so a
// negative or oversized per-lane offset needs no clamp).  (No instruction offset: an LDS-DMA adds it
// to the LDS address as well.)
__device__ __forceinline__ void dma_rs(rsrc_t r, LDSA uint8_t* row, uint32_t voff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (LDSA void*)row, 4, voff, 0, 0, 0);
}
// a buffer resource over [base, base + bytes), bytes clamped to the 32-bit record count
__device__ __forceinline__ rsrc_t rsrc_over(const void* base, uint64_t bytes) {
    return make_rsrc(base, (uint32_t)min<uint64_t>(bytes, 0xffffffffull));
}

// c ? a : b as one v_cndmask on the condition's lane mask (no branch)
__device__ __forceinline__ int vsel(bool c, int a, int b) {
    int r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(__builtin_amdgcn_ballot_w64(c)));
    return r;
}

// Where the literal kernel zstd_huf finds a frame's output.  Here the uniform geometry: frame i at byte
// i * chunk_size of `out` (zstd_ragged_decode_hip.hip has the ragged one: per-chunk pointers).  slot(): the chunk
// size the per-frame temp is laid out for; frames(): the frames of the call (the dummy area follows their temp);
// at(): per lane, the output of a frame the header kernel accepted; idle(): what a lane without a stream points at.
struct UniformOut {
    uint64_t n_total, chunk_size;
    uint8_t* out;
    __device__ __forceinline__ uint64_t slot() const { return chunk_size; }
    __device__ __forceinline__ uint64_t frames() const { return chunk_size ? (n_total + chunk_size - 1) / chunk_size : 0; }
    __device__ __forceinline__ uint8_t* at(uint64_t frame) const { return out + frame * chunk_size; }
    __device__ __forceinline__ uint8_t* idle() const { return out; }
    // the temp side: every frame's area laid out for slot() bytes, frame i's at i strides
    __device__ __forceinline__ ZLayout layout() const { return zlayout(slot()); }
    __device__ __forceinline__ const uint8_t* area(const uint8_t* zt, uint32_t frame, const ZLayout& Z) const {
        return zt + (uint64_t)frame * Z.stride;
    }
    __device__ __forceinline__ uint64_t tables(uint32_t frame, uint32_t fmin, const ZLayout& Z) const {
        return (uint64_t)(frame - fmin) * Z.stride + Z.hufs();
    }
    __device__ __forceinline__ uint8_t* dummy(uint8_t* zt, uint64_t nfr, const ZLayout& Z) const { return zt + nfr * Z.stride; }
};

}  // namespace zsplit

#ifndef LZH_DEVICE_FUNCTIONS_ONLY   // (the sequence kernel knows no output geometry: ragged batches launch it as it is)
// Sequences, one frame per lane (lanes 0 .. kFPW-1), in lock-step steps of one sequence per lane:
// ZSTD_decodeSequence (zstd_decompress_block.c:1169-1270) with the FSE tables and the bit stream in
// LDS, and every check of ZSTD_execSequence that depends on the output position (decode_block's).
// A step reads the three cells, then the sequence's four bit fields at once (offset extra bits, match
// and literal length extra bits, the three state updates: their widths are known from the cells, so
// are the positions) -- two LDS round trips per sequence, no bit container.  The steps run in
// intervals of kSB; between intervals (a uniform point, all lanes): wait for the memory operations
// issued before, flush the buffered sequences, mark the fills issued at the previous point ready,
// start blocks (raw / RLE / empty ones pass through), give the upper ring block back once the reader
// is below it, issue the fills lanes asked for -- a block's tables and 32-dword stream blocks -- as
// LDS-DMA rows masked to those lanes (no load result passes through registers: a per-lane register
// prefetch would be waited for at once, the wave's memory counter does not tell lanes apart), and
// set each lane's lowest safe position (the ready data must cover the <= 90 bits a sequence reads).
// A wave issues one instruction per 4 cycles whatever its lanes do, so the step is kept lean: no
// branches but the skip and the block's end.
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_seq_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets, uint64_t chunk_size,
                    uint32_t nchunks, int32_t* status, uint8_t* zt, const int32_t* zst, zsplit::ZFrame* zfr,
                    unsigned long long* stats, const uint32_t* flist, const uint32_t* fcnt, int which) {
    using namespace zsplit;
    using namespace zstdd;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsSeq];
    LDSA uint8_t* const S = (LDSA uint8_t*)lds;
    const int lane = threadIdx.x;
    // (the chain of one wave per SIMD is the kernel's time: its instructions go first when other kernels' waves
    // -- the literal and execution kernels beside it -- share its SIMD)
    __builtin_amdgcn_s_setprio(3);
    // frames: lane of wave blockIdx.x, or (which 0 / 1) entry of the planned short list (from the front) /
    // long list (from the back) -- lzh_zstd_plan_kernel
    const uint32_t x = blockIdx.x * kFPW + (uint32_t)lane;
    const bool inl = lane < kFPW && (which < 0 ? x < nchunks : x < fcnt[which]);
    const uint32_t f = !inl ? 0u : which < 0 ? x : (which == 0 ? flist[x] : flist[nchunks - 1 - x]);
    const bool live = inl && zst[f] == kGo;
    const ZLayout Z = zlayout(chunk_size);
    uint8_t* const zb = zt + (uint64_t)(live ? f : 0) * Z.stride;
#include "zstdd_seq_body.inc"
}
#endif   // LZH_DEVICE_FUNCTIONS_ONLY

namespace zsplit {

// one frame's output from its blocks and sequences (one wave)
__device__ __forceinline__ int exec_frame(const Bytes& rin, const Bytes& rout, const Bytes& lout, ZSink& O, LDSA uint8_t* mark,
                                          const uint8_t* zb, const ZLayout& Z, const ZFrame& fr, int lane) {
    const ZBlk* blk = (const ZBlk*)zb;
    const ZExe* ex = (const ZExe*)(zb + Z.exe());
    const uint64_t* seqs = (const uint64_t*)(zb + Z.seqs());
    ZWin fw, lw;
    fw.bind(rin, nullptr);
    int op = 0;
    for (int b = 0; b < fr.nblk; b++) {
        const uint32_t type = blk[b].type, pos = blk[b].pos, size = blk[b].size;
        if (type == 0) {
            fw.load((int)pos, lane);
            O.literals(fw, rin, (int)pos, op, (int)size, lane);
            op += (int)size;
            continue;
        }
        if (type == 1) {
            for (int base = 0; base < (int)size; base += LZH_WAVE) {
                if (base + lane < (int)size) O.put(op + base + lane, pos);
                O.maybe_flush(op + min(base + LZH_WAVE, (int)size), lane);
            }
            op += (int)size;
            continue;
        }
        const Bytes& lsrc = blk[b].ltype == 0 ? rin : lout;
        const int lpos = (int)blk[b].lit, rs = (int)blk[b].rs, nseq = (int)blk[b].nseq;
        const uint64_t* S = seqs + ex[b].seq0;
        lw.bind(lsrc, nullptr);
        lw.load(lpos, lane);
        int lp = 0;
        for (int s0 = 0; s0 < nseq;) {
            const int i = s0 + lane;
            const bool v = i < nseq;
            const uint64_t q = v ? S[i] : 0ull;
            const int ll = (int)(q & ((1u << kLenBits) - 1u)), ml = (int)((q >> kLenBits) & ((1u << kLenBits) - 1u));
            const int off = (int)(q >> (2 * kLenBits));
            const bool big = ll > 255 || ml > 4095;
            const int lin = groups::wave_incl_scan(ll);
            const int k = ffs64(ballot(!v || big || lin > 384));
            if (k > 0) {   // the first k sequences as a group
                const int o = ll + ml;
                const int oin = groups::wave_incl_scan(o);
                const int gl = rdlanei(lin, k - 1), go = rdlanei(oin, k - 1);
                const int ip = lpos + lp;
                if (!lw.covers(ip, ip + gl + 16)) lw.load(ip, lane);
                const uint64_t keep = k == LZH_WAVE ? ~0ull : ((1ull << k) - 1ull);
                groups::emit_group(lw, O, mark, ip, op, go, keep, oin - o, (uint32_t)ll | ((uint32_t)ml << 16),
                                   (uint32_t)(lin - ll), off, lane);
                op += go;
                lp += gl;
                s0 += k;
            } else {       // a long sequence on its own
                const int bl = rdlanei(ll, 0), bm = rdlanei(ml, 0), bo = rdlanei(off, 0);
                O.literals(lw, lsrc, lpos + lp, op, bl, lane);
                O.match(op + bl, bo, bm, lane);
                op += bl + bm;
                lp += bl;
                s0 += 1;
            }
        }
        const int rem = rs - lp;
        if (rem > 0) {
            O.literals(lw, lsrc, lpos + lp, op, rem, lane);
            op += rem;
        }
    }
    O.flush(op, lane);
    if (fr.ccrc >= 0) {   // ZSTD_decompressFrame's checksum check (zstd_decompress.c:1011-1020)
        wait_vm();
        fw.load(fr.ccrc, lane);
        const uint32_t want = fword(fw, fr.ccrc, lane);
        if ((uint32_t)xxh64_wave(O.out, op, lane) != want) return kErrChecksum;
    }
    return op;
}

}  // namespace zsplit

#ifndef LZH_DEVICE_FUNCTIONS_ONLY
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_hdr_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets, const uint32_t* csizes,
                    uint64_t n_total, uint64_t chunk_size, uint8_t* out, int32_t* status, uint8_t* zt, int32_t* zst,
                    zsplit::ZFrame* zfr, unsigned long long* stats, zsplit::ZHuf* jobs, uint32_t* njobs) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(zstdd::kLdsHdr + 3) / 4];
    LDSA zstdd::Lds& L = *(LDSA zstdd::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint64_t ooff = chunk * chunk_size;
    if (ooff >= n_total) return;
#include "zstdd_hdr_body.inc"
}
#endif

// Huffman literal streams, one stream per lane: 4 sections a wave (lanes 4q + j: section q, stream
// j), 8 waves per CU.  LDS: the sections' tables (2^11 cells each, rows of 16 lanes x 4 bytes as an
// LDS-DMA writes them: section q's dword d at row d / 4, lane 4q + d mod 4), the streams' bit rings
// (32 rows: stream dword d at row d mod 32, two halves of 16-dword blocks, + a mirror of row 0), the
// decoded bytes staged between flush points.  One symbol per lane per step (HUF_decodeSymbolX1: a
// tl-bit lookup, bits below the stream start read as zero); uniform points every kHB steps as in the
// sequence kernel.  A stream not consumed exactly (huf_streams' verdict 1) sends its frame to the
// one-wave decoder when the reference would use the double-symbol decoder there, else it is corrupt.
namespace zsplit {
constexpr int kHB = 16;                          // steps between uniform points (= bytes staged per lane)
// streams lzh_zstd_hufpar_kernel decodes a wave each (the rest: a lane each here)
constexpr int kParMin = 4096;                   // symbols (>= 64 bits a share)
// stream bytes staged in LDS (37 KiB a wave with the table: 4 waves per CU; a 4-stream section of 128 KiB of
// literals has streams of 32 K symbols under 8 bits each, or its literals would not be Huffman-coded)
constexpr int kParCap = 32 * 1024;
__host__ __device__ inline bool huf_par(int on, int nsym, uint32_t sz) {
    return on && nsym >= kParMin && sz + 8 <= (uint32_t)kParCap;
}
}  // namespace zsplit

// HJ sections a wave (4 HJ lanes in use).  The kernel is bound by instruction issue, not by its LDS round
// trips: 8 sections a wave (36 KiB of LDS, one wave per SIMD) issue half the instructions per section of
// 4 a wave (two waves per SIMD) -- 1 GiB -b128: mixed 5.3 -> 4.9 ms, text 2.0 -> 1.6 ms; 2 a wave 6.5 /
// 3.2 ms -- but need 32 sections per CU to keep every SIMD busy, so launches with fewer frames keep 4.
// G: the output geometry (zsplit::UniformOut, or the ragged one)
template <int HJ, class G>
__device__ __forceinline__ void zstd_huf(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                         const G& g, int32_t* status, uint8_t* zt, int32_t* zst,
                                         const zsplit::ZHuf* jobs, const uint32_t* njobs, unsigned long long* stats,
                                         int par) {
    using namespace zsplit;
    using namespace zstdd;
    constexpr int kHJ = HJ, kHL = 4 * kHJ;          // sections a wave, lanes in use
    constexpr int kHRow = 4 * kHL;                   // bytes per LDS row (one dword per lane in use)
    constexpr int kHLdsRing = 256 * kHRow, kHLds = kHLdsRing + 33 * kHRow;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kHLds];
    LDSA uint8_t* const S = (LDSA uint8_t*)lds;
    const int lane = threadIdx.x;
    const int q = lane >> 2, j = lane & 3;
    const uint32_t jid = blockIdx.x * kHJ + (uint32_t)q;
    const bool jlive = lane < kHL && jid < *njobs;
    uint32_t jf = 0, jtblk = 0, jtl = 0, jx2 = 0, jns = 0, jdst = 0, jseg = 0, jlast = 0, js0 = 0, jsz = 0;
    if (jlive) {
        const ZHuf* J = jobs + jid;
        jf = J->frame; jtblk = J->tblk; jtl = J->tl; jx2 = J->x2; jns = J->ns; jdst = J->dst; jseg = J->seg;
        jlast = J->last; js0 = J->s0[j]; jsz = J->sz[j];
    }
    bool slive = jlive && zst[jf] == kGo && (uint32_t)j < jns &&
                 !huf_par(par, j == 3 ? (int)jlast : (int)jseg, jsz);   // (long streams: lzh_zstd_hufpar_kernel)
    const ZLayout Z = g.layout();   // (the uniform slots' layout; the compact geometry has one per frame)
    // resources from the wave's lowest frame: the packed streams and the table slots (per-lane 32-bit
    // offsets; a section whose offsets would not fit goes to the one-wave decoder).  g.area(): a frame's temp area;
    // g.tables(): the offset of a frame's Huffman table slots from the lowest frame's area (areas rise with the
    // frame index in every geometry); g.dummy(): the dummy words
    uint32_t fmin = jlive ? jf : 0xffffffffu;
    for (int k = 1; k < 64; k <<= 1) fmin = min(fmin, (uint32_t)__shfl_xor((int)fmin, k));
    fmin = uni(fmin == 0xffffffffu ? 0u : fmin);
    const int64_t readable = (int64_t)packed_readable;
    const uint8_t* zb0 = g.area(zt, fmin, Z);
    const rsrc_t rz = rsrc_over(zb0, (uint64_t)0xffffffffull);
    const uint64_t toff = g.tables(jf, fmin, Z) + (uint64_t)jtblk * kHufSlot;
    bool far_ = jlive && toff + kHufSlot > 0xffffffffull;
    const uint64_t nfr = g.frames();
    uint8_t* const dummy = g.dummy(zt, nfr, Z) + (64ull * blockIdx.x) % zdummy_bytes(nfr);   // (spread like the seq kernel's)
    const int l4 = lane * 4;
    const int tl = (int)jtl;
    // this lane's stream
    int P = 0, lo = 0, nsym = 0, done = 0;
    int64_t A = 0;
    uint8_t* dst = g.idle();
    if (slive) {
        const int64_t s0 = (int64_t)offsets[jf] + (int64_t)js0;
        A = s0 & ~3ll;

        const int x0 = (int)(s0 & 3), X = x0 + (int)jsz - 1;
        lo = 8 * x0;
        P = 8 * X + hb32((uint32_t)packed[A + X]);   // (the end mark: checked non-zero by the header kernel)
        nsym = j == 3 ? (int)jlast : (int)jseg;
        dst = g.at(jf) + jdst + (uint64_t)j * jseg;
    }
    int hb0 = 0, hb1 = 0, rdy = 0, req = 0, iss = 0;
    {
        const int bt = (P - 1) >> 9;
        hb0 = (bt & 1) ? bt - 1 : bt;
        hb1 = (bt & 1) ? bt : bt - 1;
        req = slive ? 3 : 0;
    }
    {   // (a section whose offsets do not fit: its frame goes to the one-wave decoder)
        const uint64_t fm = ballot(far_);
        if (fm) {
            const bool qfar = ((fm >> (4 * q)) & 15ull) != 0;
            if (qfar && j == 0 && jlive) atomicMax(&zst[jf], kLegacy);
            slive = slive && !qfar;
        }
    }
    int res = 0;                                  // 0 going, 1 exact, 2 not exact
    auto fld = [&](int bq, int w) -> uint32_t {
        const LDSA uint8_t* a = S + kHLdsRing + ((bq >> 5) & 31) * kHRow + l4;
        const uint32_t v = __builtin_amdgcn_alignbit(*(const LDSA uint32_t*)(a + kHRow), *(const LDSA uint32_t*)a,
                                                     (uint32_t)bq & 31u);
        return __builtin_amdgcn_ubfe(v, 0u, (uint32_t)w);
    };
    if (!slive) req = 0;
    bool going = slive;
    int lowok = 1 << 30;                         // a step runs while P >= lowok (the ready blocks + tl bits)
    uint64_t hst[5] = {0, 0, 0, 0, 0}, tmark = 0;   // (LZH_ZSTD_STATS: points, steps, intervals, waits, symbols)
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    for (int ival = 0;; ival++) {
        if (LZH_ZSTD_STATS) {
            const uint64_t t = __builtin_amdgcn_s_memtime();
            if (ival) hst[1] += t - tmark;
            tmark = t;
            hst[2]++;
        }
        // ---- uniform point: every memory operation but the last interval's kHB byte stores is done
        __builtin_amdgcn_s_waitcnt(vmcnt_imm(kHB));
        if (LZH_ZSTD_STATS) hst[3] += __builtin_amdgcn_s_memtime() - tmark;
        rdy |= iss;
        iss = 0;
        if (going && done == nsym) {             // huf_streams' verdict: exactly consumed
            res = P == lo ? 1 : 2;
            going = false;
        }
        if (going) {   // the upper block, once the reader is below it, takes the block under the lower one
            const int top = (P - 1) >> 9;
            if ((rdy & 1) && hb0 > top && hb0 > hb1) { hb0 = hb1 - 1; rdy &= ~1; req |= 1; }
            if ((rdy & 2) && hb1 > top && hb1 > hb0) { hb1 = hb0 - 1; rdy &= ~2; req |= 2; }
        }
        if (ival == 0 && ballot(jlive)) {   // the sections' tables: row r = dwords 4r .. 4r+3
            if (jlive) {
                const uint32_t o = (uint32_t)toff + 4 * j;
#pragma unroll 1
                for (int r = 0; r < 256; r += 16) {
                    LDSA uint8_t* d = S + r * kHRow;
                    const uint32_t orr = o + 16 * r;
                    dma_rs(rz, d, orr); dma_rs(rz, d + kHRow, orr + 16); dma_rs(rz, d + 2 * kHRow, orr + 32);
                    dma_rs(rz, d + 3 * kHRow, orr + 48); dma_rs(rz, d + 4 * kHRow, orr + 64);
                    dma_rs(rz, d + 5 * kHRow, orr + 80); dma_rs(rz, d + 6 * kHRow, orr + 96);
                    dma_rs(rz, d + 7 * kHRow, orr + 112); dma_rs(rz, d + 8 * kHRow, orr + 128);
                    dma_rs(rz, d + 9 * kHRow, orr + 144); dma_rs(rz, d + 10 * kHRow, orr + 160);
                    dma_rs(rz, d + 11 * kHRow, orr + 176); dma_rs(rz, d + 12 * kHRow, orr + 192);
                    dma_rs(rz, d + 13 * kHRow, orr + 208); dma_rs(rz, d + 14 * kHRow, orr + 224);
                    dma_rs(rz, d + 15 * kHRow, orr + 240);
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (ballot(req & (1 << h))) {   // the block's 16 dwords (global_load_lds rows: see the sequence kernel)
                const int64_t x0 = A + 64ll * (h ? hb1 : hb0);
                // a block wholly outside the packed bytes holds no stream data: any readable bytes will do
                const bool part = x0 >= 0 && x0 < readable && x0 + 64 > readable;
                const uint8_t* g = packed + (x0 < 0 || x0 >= readable ? 0 : x0);
                LDSA uint8_t* d = S + kHLdsRing + h * 16 * kHRow;
                if ((req & (1 << h)) && !part) {
#pragma unroll
                    for (int k = 0; k < 16; k++) dma_row(g + 4 * k, d + k * kHRow);
                    if (h == 0) dma_row(g, S + kHLdsRing + 32 * kHRow);   // (the mirror of row 0)
                }
                if (ballot((req & (1 << h)) && part)) {   // (the packed bytes end inside the block)
                    if ((req & (1 << h)) && part) {
                        for (int k = 0; k < 16; k++)
                            dma_row(packed + (x0 + 4 * k < readable - 4 ? x0 + 4 * k : ((readable - 4) & ~3ll)), d + k * kHRow);
                        if (h == 0) dma_row(packed + x0, S + kHLdsRing + 32 * kHRow);
                    }
                }
                if (req & (1 << h)) {
                    req &= ~(1 << h);
                    iss |= 1 << h;
                }
            }
        }
        lowok = (rdy == 3 ? 512 * min(hb0, hb1) : (rdy == 1 ? 512 * hb0 : (rdy == 2 ? 512 * hb1 : (1 << 30)))) + 12;
        if (!going) lowok = 1 << 30;
        if (LZH_ZSTD_STATS) {
            const uint64_t t = __builtin_amdgcn_s_memtime();
            hst[0] += t - tmark;
            tmark = t;
        }
        if (!ballot(going)) break;
        if (ival > 2 * kBlockMax) {   // (a bound every stream meets)
            if (going) { going = false; res = 2; }
            lowok = 1 << 30;
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- kHB steps, one symbol each (HUF_decodeSymbolX1) and exactly one byte store per lane (a dummy
        // byte for a lane without a symbol), so that the next point's vmcnt(kHB) waits for the fills only
#pragma unroll 2
        for (int k = 0; k < kHB; k++) {
            const bool act = P >= lowok && done < nsym;
            const int bq = P - tl;
            uint32_t v = fld(bq, tl);
            if (bq < lo) v &= lo - bq >= 32 ? 0u : (~0u << (lo - bq));   // (zero-padded below the start)
            const uint32_t e = *(const LDSA uint16_t*)(S + (v >> 3) * kHRow + (q << 4) + (v & 7) * 2);
            *(act ? dst + done : dummy + lane) = (uint8_t)e;
            P -= act ? (int)(e >> 8) : 0;
            done += act;
        }
    }
    if (LZH_ZSTD_STATS && stats && lane == 0) {
        for (int k = 0; k < 4; k++) atomicAdd(&stats[k], (unsigned long long)hst[k]);
    }
    if (LZH_ZSTD_STATS && stats && slive) atomicAdd(&stats[4], (unsigned long long)nsym);
    if (LZH_ZSTD_STATS && stats && slive && res == 2) atomicAdd(&stats[5 + (int)jx2], 1ull);
    if (LZH_ZSTD_STATS && stats && far_) atomicAdd(&stats[7], 1ull);
    if (slive && res == 2) {   // not consumed exactly: X2's verdict (the one-wave decoder) or corrupt
        if (jx2) {
            atomicMax(&zst[jf], kLegacy);
        } else if (atomicMax(&zst[jf], kDone) != kDone) {
            status[jf] = ZC;
        }
    }
}

// Long Huffman streams, one per WAVE (self-synchronising parallel decode).  A 4-stream literal section of a
// frame with few matches holds up to 32 K symbols a stream, and one lane's serial decode of it -- two
// dependent LDS round trips a symbol -- bounds lzh_zstd_huf_kernel (config 5's 512 MiB share: a third of
// the frames are whole-block literals).  Here the stream's bits are cut into 64 equal shares, one per lane:
// every lane decodes its share from its top (lane 0 from the stream's start, the others from a guess),
// recording where its chain leaves the share and how many symbols it took; a lane whose true start -- the
// previous lane's exit -- differs from the one it used decodes again from there (Huffman codes
// resynchronise within a few symbols, so after one such round the exits no longer move); the symbol
// counts' prefix sum places every share's output, and a last pass writes it.  The chain from the stream's
// start is the serial decoder's, so the verdict is huf_streams': exact iff it ends exactly at the start of
// the stream's bits after exactly nsym symbols (else the frame goes to the one-wave decoder (X2) or is
// corrupt, as in lzh_zstd_huf_kernel).

#ifndef LZH_DEVICE_FUNCTIONS_ONLY   // (the rest of the file: the uniform kernels, the launchers)
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_hufpar_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets, uint64_t chunk_size,
                       uint8_t* out, int32_t* status, uint8_t* zt, int32_t* zst, const zsplit::ZHuf* jobs,
                       const uint32_t* njobs, int par) {
#include "zstdd_hufpar_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_huf_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets, uint64_t n_total,
                    uint64_t chunk_size, uint8_t* out, int32_t* status, uint8_t* zt, int32_t* zst,
                    const zsplit::ZHuf* jobs, const uint32_t* njobs, unsigned long long* stats, int par) {
    zstd_huf<4>(packed, packed_readable, offsets, zsplit::UniformOut{n_total, chunk_size, out}, status, zt, zst, jobs,
                njobs, stats, par);
}
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_huf8_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets, uint64_t n_total,
                     uint64_t chunk_size, uint8_t* out, int32_t* status, uint8_t* zt, int32_t* zst,
                     const zsplit::ZHuf* jobs, const uint32_t* njobs, unsigned long long* stats, int par) {
    zstd_huf<8>(packed, packed_readable, offsets, zsplit::UniformOut{n_total, chunk_size, out}, status, zt, zst, jobs,
                njobs, stats, par);
}

// The sequence / execution plan: frames the header and literal kernels left at kGo, split by their sequence
// count -- long (nsq > max / 2) at the back of `flist`, short at the front, each in frame order -- so that the
// execution of the short frames runs while the long ones still decode (the sequence kernel's time is its
// longest chains').  One workgroup of 1024 threads; fcnt = {short, long}.
extern "C" __global__ void __launch_bounds__(1024)
lzh_zstd_plan_kernel(const int32_t* zst, const zsplit::ZFrame* zfr, uint32_t nchunks, uint32_t* flist, uint32_t* fcnt) {
    __shared__ uint32_t smax, wsum[2][16], base[2];
    const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
    if (t == 0) { smax = 0; base[0] = 0; base[1] = 0; }
    __syncthreads();
    uint32_t m = 0;
    for (uint32_t i = t; i < nchunks; i += 1024)
        if (zst[i] == zsplit::kGo) m = max(m, (uint32_t)max(zfr[i].nsq, 0));
    atomicMax(&smax, m);
    __syncthreads();
    const uint32_t thr = smax / 2;
    for (uint32_t i0 = 0; i0 < nchunks; i0 += 1024) {
        const uint32_t i = i0 + t;
        const bool go = i < nchunks && zst[i] == zsplit::kGo;
        const bool lng = go && (uint32_t)max(zfr[i].nsq, 0) > thr;
        const uint64_t bs = __builtin_amdgcn_ballot_w64(go && !lng), bl = __builtin_amdgcn_ballot_w64(lng);
        const uint64_t below = (1ull << lane) - 1ull;
        if (lane == 0) { wsum[0][w] = (uint32_t)__builtin_popcountll(bs); wsum[1][w] = (uint32_t)__builtin_popcountll(bl); }
        __syncthreads();
        uint32_t ps = base[0], pl = base[1];
        for (uint32_t k = 0; k < w; k++) { ps += wsum[0][k]; pl += wsum[1][k]; }
        if (go && !lng) flist[ps + (uint32_t)__builtin_popcountll(bs & below)] = i;
        if (lng) flist[nchunks - 1 - (pl + (uint32_t)__builtin_popcountll(bl & below))] = i;
        __syncthreads();
        if (t == 0)
            for (uint32_t k = 0; k < 16; k++) { base[0] += wsum[0][k]; base[1] += wsum[1][k]; }
        __syncthreads();
    }
    if (t == 0) {
        // the long list rounded up to whole sequence waves with the short list's last frames, so that the two
        // launches' frames need no more waves than one launch's (a wave more than there are SIMDs would wait
        // for a whole chain); the ranges are disjoint or the entries already in place (see the indices)
        uint32_t ns = base[0], nl = base[1];
        const uint32_t m = min((uint32_t)(zsplit::kFPW - nl % zsplit::kFPW) % zsplit::kFPW, ns);
        for (uint32_t j = 0; j < m; j++) flist[nchunks - 1 - (nl + j)] = flist[ns - 1 - j];
        fcnt[0] = ns - m;
        fcnt[1] = nl + m;
    }
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_exec_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets, const uint32_t* csizes,
                     uint64_t n_total, uint64_t chunk_size, uint8_t* out, int32_t* status, const uint8_t* zt,
                     int32_t* zst, const zsplit::ZFrame* zfr, const uint32_t* flist, const uint32_t* fcnt, int which,
                     uint32_t nchunks) {
    __shared__ __attribute__((aligned(16))) uint8_t win[zstdd::kZW + 3 * LZH_WAVE];
    const int lane = threadIdx.x;
    if (which >= 0 && blockIdx.x >= fcnt[which]) return;
    const uint64_t chunk = which < 0 ? blockIdx.x : (which == 0 ? flist[blockIdx.x] : flist[nchunks - 1 - blockIdx.x]);
    const uint64_t ooff = chunk * chunk_size;
    if (ooff >= n_total || zst[chunk] != zsplit::kGo) return;   // (the header / literal kernels' verdict first)
#include "zstdd_exec_body.inc"
}

extern "C" __global__ void __launch_bounds__(64, LZH_ZSTD_MINW)
lzh_zstd_decompress_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                           const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size, uint8_t* out,
                           int32_t* status, uint32_t chunk0, unsigned long long* stats, const int32_t* zsel) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(sizeof(zstdd::Lds) + 3) / 4];
    LDSA zstdd::Lds& L = *(LDSA zstdd::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t chunk = (uint64_t)blockIdx.x + chunk0;
    const uint64_t ooff = chunk * chunk_size;
    if (ooff >= n_total) return;
    if (zsel && zsel[chunk] != zsplit::kLegacy) return;   // (decoded by the split kernels)
    const int part = (int)min(chunk_size, n_total - ooff);
#include "zstdd_frame_body.inc"
}

#include "launch.h"

#include <mutex>
// Test hook: force the LZ4 / snappy decoder's output window (4096, 8192 or 16384; 0 = by chunk count)
// so that the parity tests run every window kernel on the same streams.
static int g_force_window = 0;
// Test hook: 1 = decode zstd frames with the one-wave-per-frame kernel only (no split kernels)
static int g_zstd_legacy = 0;
extern "C" int lzh_debug_zstd_legacy(int on) {
    g_zstd_legacy = on ? 1 : 0;
    return 0;
}
// Test hook: force the zstd literal kernel's sections per wave (4 or 8; 0 = by frame count)
// Test hook: long Huffman streams one per wave (lzh_zstd_hufpar_kernel) on / off
// the sequence kernel on a per-device side stream beside the literal kernels (0: all on the caller's stream)
static int g_zstd_side = 1;
extern "C" int lzh_debug_zstd_side(int on) {
    g_zstd_side = on ? 1 : 0;
    return 0;
}
// Side streams per caller stream (and per slot k): independent callers -- the batched rows' two alternating
// kernel streams, other threads' streams -- never queue behind each other's forked kernels.  Each entry owns its
// fork / join events (a call records and waits them on its own caller stream, in order).  A caller stream on a
// device other than the current one, or past kMaxSide entries, gets no side stream: the caller then launches
// everything on its own stream, in order.
struct SideEntry {
    hipStream_t caller;
    int dev, k;
    hipStream_t ss;
    hipEvent_t fork, join;
};
static constexpr int kMaxSide = 256;
static SideEntry g_side[kMaxSide];
static int g_nside = 0;
static std::mutex g_side_mu;
bool lzh_side_stream(hipStream_t s, hipStream_t& ss, hipEvent_t& fork, hipEvent_t& join, int k) {
    if (k < 0 || k > 1) return false;
    int dev = -1, sdev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    hipDevice_t d = 0;
    if (hipStreamGetDevice(s, &d) != hipSuccess) return false;
    sdev = (int)d;
    if (sdev != dev) return false;
    std::lock_guard<std::mutex> g(g_side_mu);
    for (int i = 0; i < g_nside; i++)
        if (g_side[i].caller == s && g_side[i].dev == dev && g_side[i].k == k) {
            ss = g_side[i].ss;
            fork = g_side[i].fork;
            join = g_side[i].join;
            return true;
        }
    if (g_nside >= kMaxSide) return false;
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) hi = 0;
    SideEntry e{s, dev, k, nullptr, nullptr, nullptr};
    // (the highest priority: their waves go out before the caller's stream's)
    if (hipStreamCreateWithPriority(&e.ss, hipStreamNonBlocking, hi) != hipSuccess) return false;
    if (hipEventCreateWithFlags(&e.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e.join, hipEventDisableTiming) != hipSuccess) {
        if (e.fork) (void)hipEventDestroy(e.fork);
        (void)hipStreamDestroy(e.ss);
        return false;
    }
    g_side[g_nside++] = e;
    ss = e.ss;
    fork = e.fork;
    join = e.join;
    return true;
}
// (tests: how many side streams the library holds)
extern "C" int lzh_debug_side_streams() {
    std::lock_guard<std::mutex> g(g_side_mu);
    return g_nside;
}
// the sequence / execution plan by sequence count (lzh_zstd_plan_kernel; 0: one sequence launch)
static int g_zstd_plan = 1;
extern "C" int lzh_debug_zstd_plan(int on) {
    g_zstd_plan = on ? 1 : 0;
    return 0;
}
static int g_zstd_hufpar = 1;
extern "C" int lzh_debug_zstd_hufpar(int on) {
    g_zstd_hufpar = on ? 1 : 0;
    return 0;
}
static int g_zstd_huf_sections = 0;
extern "C" int lzh_debug_zstd_huf_sections(int hj) {
    if (hj != 0 && hj != 4 && hj != 8) return -1;
    g_zstd_huf_sections = hj;
    return 0;
}
// the current device's CUs (0: unknown)
static int zstd_cus() {
    static int hcus[64];
    int hdev = 0;
    (void)hipGetDevice(&hdev);
    if (hdev < 0 || hdev >= 64) hdev = 0;
    if (!hcus[hdev] && hipDeviceGetAttribute(&hcus[hdev], hipDeviceAttributeMultiprocessorCount, hdev) != hipSuccess)
        hcus[hdev] = 0;
    return hcus[hdev];
}
// Huffman sections a wave for a launch of nchunks frames
// (8 sections a wave once the frames -- about one Huffman job each -- fill 8 x 4 waves per CU)
static int zstd_huf_sections(uint32_t nchunks) {
    const int cus = zstd_cus();
    return (g_zstd_huf_sections ? g_zstd_huf_sections == 8 : cus > 0 && (uint64_t)nchunks >= 32ull * (uint64_t)cus) ? 8 : 4;
}
// (the ragged launcher of zstd_ragged_decode_hip.hip: the same hooks, the same rule)
LzhZstdHooks lzh_zstd_hooks(uint32_t nchunks) { return {g_zstd_legacy, g_zstd_hufpar, zstd_huf_sections(nchunks)}; }
extern "C" int lzh_debug_force_decode_window(int kw) {
    if (kw != 0 && kw != 4096 && kw != 8192 && kw != 16384) return -1;
    g_force_window = kw;
    return 0;
}

// The LZ4 / snappy decoder's LDS output window for a launch of nchunks on the current device: the
// widest whose occupancy (waves per CU by LDS: 160 KiB in 512-byte granules, at most 32 waves) still
// holds every chunk at once; 4096 = lzh_decompress_v2_kernel, 8192 = _w8k, 16384 = _w16k.
static int decode_window(uint32_t nchunks) {
    if (g_force_window) return g_force_window;
    static int cus[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus[dev] = 0;
    auto fits = [&](int kw) {
        const int lds = (kw + 3 * LZH_WAVE + kRingBytes + 511) / 512 * 512;
        return (uint64_t)nchunks <= (uint64_t)cus[dev] * (uint64_t)min(32, 160 * 1024 / lds);
    };
    if (LZH_DEC_WIDE && cus[dev] > 0) {
        if (LZH_DEC_WIDE >= 2 && fits(16384)) return 16384;
        if (fits(8192)) return 8192;
    }
    return 4096;
}
// (bench.py names the decode kernel a launch of nchunks runs)
extern "C" int lzh_debug_decode_window(uint32_t nchunks) { return decode_window(nchunks); }

hipError_t lzh_launch_decompress(int codec, const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                 const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size, uint8_t* out,
                                 int32_t* status, uint32_t nchunks, hipStream_t s, const void* desc) {
    if (nchunks == 0) return hipSuccess;
    const int kw = decode_window(nchunks);
    auto k = kw == 16384 ? lzh_decompress_w16k_kernel : kw == 8192 ? lzh_decompress_w8k_kernel : lzh_decompress_v2_kernel;
    hipLaunchKernelGGL(k, dim3(nchunks), dim3(64), 0, s, codec, packed, packed_readable, offsets, csizes, n_total,
                       chunk_size, out, status, 0u, (const uint32_t*)desc);
    if (desc && codec == 0)   // LZ4 frames: the linked ones (descriptors the kernel above skipped)
        hipLaunchKernelGGL(lzh_decompress_linked_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, out,
                           status, (const uint32_t*)desc);
    return hipGetLastError();
}

// The split pays where a chunk's serial decode is long against the walk: from 8 fragments (512 KiB)
// (mixed 1 GiB: -b256 walk 3.1 + fragments 3.3 ms against 6.5 ms whole; -b1024 9.2 + 3.4 against 18.5 ms;
// profiles/r05_snsplit).  Test hooks: the mode (0 off: every chunk whole; 1 from kMinFrags fragments;
// 2 from 2 fragments), and the number of chunks finished by fragments (reset with reset != 0).
static int g_snappy_split = 1;
extern "C" int lzh_debug_snappy_split(int mode) {
    if (mode < 0 || mode > 2) return -1;
    g_snappy_split = mode;
    return 0;
}
extern "C" long long lzh_debug_snappy_split_done(int reset) {
    unsigned long long v = 0;
    if (reset) return hipMemcpyToSymbol(HIP_SYMBOL(lzh_snsplit_done), &v, sizeof(v)) == hipSuccess ? 0 : -1;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(lzh_snsplit_done), sizeof(v)) != hipSuccess) return -1;
    return (long long)v;
}

// temp for the fragment-parallel snappy decode (0: chunks of one fragment, or too large to split):
// fragment descriptors (32 B) and statuses, per-chunk split flags and whole-chunk descriptors
size_t lzh_snappy_split_temp(uint64_t n, uint64_t chunk_size) {
    const uint32_t F = snsplit::frags(chunk_size);
    if (!g_snappy_split || F < (g_snappy_split == 2 ? 2u : snsplit::kMinFrags) || F > snsplit::kMaxFrags || n == 0)
        return 0;
    const uint64_t k = (n + chunk_size - 1) / chunk_size;
    auto al = [](uint64_t v) { return (v + 255) & ~(uint64_t)255; };
    return (size_t)(al(k * F * 32) + al(k * F * 4) + al(k * 4) + al(k * 32) + 256);
}

hipError_t lzh_launch_snappy_split_decompress(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                              const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size, uint8_t* out,
                                              int32_t* status, uint32_t nchunks, uint8_t* temp, hipStream_t s) {
    if (nchunks == 0) return hipSuccess;
    const uint32_t F = snsplit::frags(chunk_size);
    const uint64_t k = nchunks;
    auto al = [](uint64_t v) { return (v + 255) & ~(uint64_t)255; };
    uint32_t* desc = (uint32_t*)temp;
    int32_t* fstat = (int32_t*)(temp + al(k * F * 32));
    uint32_t* cflag = (uint32_t*)(temp + al(k * F * 32) + al(k * F * 4));
    uint32_t* sdesc = (uint32_t*)(temp + al(k * F * 32) + al(k * F * 4) + al(k * 4));
    if (k * F > 0xffffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lzh_snappy_split_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets, csizes,
                       n_total, chunk_size, F, desc, cflag);
    hipError_t e = lzh_launch_decompress(1, packed, packed_readable, nullptr, nullptr, n_total, chunk_size, out, fstat,
                                         (uint32_t)(k * F), s, desc);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzh_snappy_join_kernel, dim3((nchunks + 255) / 256), dim3(256), 0, s, offsets, csizes, n_total,
                       chunk_size, F, desc, fstat, cflag, sdesc, status, nchunks);
    return lzh_launch_decompress(1, packed, packed_readable, nullptr, nullptr, n_total, chunk_size, out, status, nchunks,
                                 s, sdesc);
}

hipError_t lzh_launch_zstd_decompress(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                      const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size, uint8_t* out,
                                      int32_t* status, uint32_t nchunks, uint8_t* zt, hipStream_t s) {
    if (nchunks == 0) return hipSuccess;
    unsigned long long* stats = nullptr;
#if LZH_ZSTD_STATS
    static unsigned long long* d_stats = nullptr;
    if (!d_stats) (void)hipMalloc(&d_stats, zstdd::kZClk * sizeof(unsigned long long));
    (void)hipMemsetAsync(d_stats, 0, zstdd::kZClk * sizeof(unsigned long long), s);
    stats = d_stats;
#endif
    const int32_t* zsel = nullptr;
    if (zt && !g_zstd_legacy) {   // the split kernels; frames they leave go to the one-wave decoder below
        const zsplit::ZLayout Z = zsplit::zlayout(chunk_size);
        int32_t* zst = (int32_t*)(zt + (uint64_t)nchunks * Z.stride + zsplit::zdummy_bytes(nchunks));   // (after the dummy words)
        zsplit::ZFrame* zfr = (zsplit::ZFrame*)((uint8_t*)zst + (((uint64_t)nchunks * 4 + 255) & ~255ull));
        uint32_t* njobs = (uint32_t*)((uint8_t*)zfr + (((uint64_t)nchunks * sizeof(zsplit::ZFrame) + 255) & ~255ull));
        zsplit::ZHuf* jobs = (zsplit::ZHuf*)((uint8_t*)njobs + 256);
        (void)hipMemsetAsync(njobs, 0, 4, s);
        hipLaunchKernelGGL(lzh_zstd_hdr_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets, csizes,
                           n_total, chunk_size, out, status, zt, zst, zfr, stats, jobs, njobs);
        // the sequence kernel needs the header kernel's output only (its verdict goes to zfr[].sv): it runs
        // on a side stream beside the literal kernels, launched first -- its waves, one per SIMD at config 5's
        // share, take their SIMDs and the literal waves fill the rest -- and the execution kernel joins both
        // and after the plan (lzh_zstd_plan_kernel) the frames with the longest sequence chains decode on one
        // side stream, the rest on another, so that the execution kernel runs the short ones while the long
        // ones still decode
        uint32_t* flist = (uint32_t*)((uint8_t*)jobs + (uint64_t)nchunks * Z.bmax * sizeof(zsplit::ZHuf) + 256);
        uint32_t* fcnt = flist + nchunks;
        hipStream_t sq[2] = {s, s};
        hipEvent_t fork[2] = {nullptr, nullptr}, join[2] = {nullptr, nullptr};
        const bool side = !LZH_ZSTD_STATS && g_zstd_side && lzh_side_stream(s, sq[0], fork[0], join[0], 0) &&
                          lzh_side_stream(s, sq[1], fork[1], join[1], 1);
        const unsigned sgrid = (nchunks + zsplit::kFPW - 1) / zsplit::kFPW;
        const int cus = zstd_cus();
        // (the plan only while the sequence waves leave LDS room beside them -- at most 2 of a CU's 4 -- for the
        // literal kernels, whose end the execution of the short frames waits for; else one sequence launch)
        const bool plan = side && g_zstd_plan && cus > 0 && sgrid <= 2u * (unsigned)cus;
        if (plan) {
            hipLaunchKernelGGL(lzh_zstd_plan_kernel, dim3(1), dim3(1024), 0, s, (const int32_t*)zst,
                               (const zsplit::ZFrame*)zfr, nchunks, flist, fcnt);
            for (int k = 0; k < 2; k++) {   // long list (which 1) on side stream 0, launched first
                (void)hipEventRecord(fork[k], s);
                (void)hipStreamWaitEvent(sq[k], fork[k], 0);
                hipLaunchKernelGGL(lzh_zstd_seq_kernel, dim3(sgrid), dim3(64), 0, sq[k], packed, packed_readable,
                                   offsets, chunk_size, nchunks, status, zt, zst, zfr, nullptr, (const uint32_t*)flist,
                                   (const uint32_t*)fcnt, 1 - k);
                (void)hipEventRecord(join[k], sq[k]);
            }
        } else if (side) {
            (void)hipEventRecord(fork[0], s);
            (void)hipStreamWaitEvent(sq[0], fork[0], 0);
            hipLaunchKernelGGL(lzh_zstd_seq_kernel, dim3(sgrid), dim3(64), 0, sq[0], packed, packed_readable, offsets,
                               chunk_size, nchunks, status, zt, zst, zfr, nullptr, (const uint32_t*)nullptr,
                               (const uint32_t*)nullptr, -1);
            (void)hipEventRecord(join[0], sq[0]);
        }
        const uint64_t maxjobs = (uint64_t)nchunks * Z.bmax;
        unsigned long long* hstats = nullptr;
#if LZH_ZSTD_STATS
        static unsigned long long* d_hst = nullptr;
        if (!d_hst) (void)hipMalloc(&d_hst, 8 * sizeof(unsigned long long));
        (void)hipMemsetAsync(d_hst, 0, 8 * sizeof(unsigned long long), s);
        hstats = d_hst;
#endif
        const int hj = zstd_huf_sections(nchunks);
        hipLaunchKernelGGL(hj == 8 ? lzh_zstd_huf8_kernel : lzh_zstd_huf_kernel, dim3((unsigned)((maxjobs + hj - 1) / hj)),
                           dim3(64), 0, s, packed, packed_readable, offsets, n_total, chunk_size, out, status, zt, zst,
                           (const zsplit::ZHuf*)jobs, (const uint32_t*)njobs, hstats, g_zstd_hufpar);
        if (g_zstd_hufpar)   // (off: the per-lane kernel above decoded every stream)
            hipLaunchKernelGGL(lzh_zstd_hufpar_kernel, dim3((unsigned)(maxjobs * 4)), dim3(64), 0, s, packed,
                               packed_readable, offsets, chunk_size, out, status, zt, zst, (const zsplit::ZHuf*)jobs,
                               (const uint32_t*)njobs, g_zstd_hufpar);
#if LZH_ZSTD_STATS
        {
            unsigned long long h[8];
            uint32_t nj = 0;
            (void)hipMemcpyAsync(h, d_hst, sizeof(h), hipMemcpyDeviceToHost, s);
            (void)hipMemcpyAsync(&nj, njobs, 4, hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            const double w = (double)((nj + hj - 1) / hj);
            fprintf(stderr, "zstd huf kernel: %u sections, %.0f symbols a stream; per wave: intervals %.0f; clocks per "
                            "interval: uniform point %.0f (its wait %.0f), steps %.0f; inexact streams %llu (x1) %llu (x2), "
                            "far %llu\n",
                    nj, (double)h[4] / (nj ? 4.0 * nj : 1.0), h[2] / (w ? w : 1), (double)h[0] / (h[2] ? h[2] : 1),
                    (double)h[3] / (h[2] ? h[2] : 1), (double)h[1] / (h[2] ? h[2] : 1), h[5], h[6], h[7]);
        }
#endif
        unsigned long long* sstats = nullptr;
#if LZH_ZSTD_STATS
        static unsigned long long* d_sst = nullptr;
        if (!d_sst) (void)hipMalloc(&d_sst, 16 * sizeof(unsigned long long));
        (void)hipMemsetAsync(d_sst, 0, 16 * sizeof(unsigned long long), s);
        sstats = d_sst;
#endif
        if (!side)
            hipLaunchKernelGGL(lzh_zstd_seq_kernel, dim3(sgrid), dim3(64), 0, s, packed, packed_readable, offsets,
                               chunk_size, nchunks, status, zt, zst, zfr, sstats, (const uint32_t*)nullptr,
                               (const uint32_t*)nullptr, -1);
#if LZH_ZSTD_STATS
        {
            unsigned long long h[16];
            (void)hipMemcpyAsync(h, d_sst, sizeof(h), hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            const double w = (double)((nchunks + zsplit::kFPW - 1) / zsplit::kFPW);
            fprintf(stderr, "zstd seq kernel per wave: intervals %.0f (with block starts %.0f), steps %.0f; clocks per "
                            "interval: uniform point %.0f (its wait %.0f), steps %.0f; frames to the one-wave decoder %llu; clock %.0f MHz\n",
                    h[2] / w, h[3] / w, h[4] / w, (double)h[0] / h[2], (double)h[5] / h[2], (double)h[1] / h[2], h[6],
                    100.0 * (double)h[8] / (double)(h[9] ? h[9] : 1));
        }
#endif
        if (plan) {
            for (int k = 1; k >= 0; k--) {   // the short list once its sequences are done, then the long one
                (void)hipStreamWaitEvent(s, join[k], 0);
                hipLaunchKernelGGL(lzh_zstd_exec_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets,
                                   csizes, n_total, chunk_size, out, status, zt, zst, zfr, (const uint32_t*)flist,
                                   (const uint32_t*)fcnt, 1 - k, nchunks);
            }
        } else {
            if (side) (void)hipStreamWaitEvent(s, join[0], 0);
            hipLaunchKernelGGL(lzh_zstd_exec_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets,
                               csizes, n_total, chunk_size, out, status, zt, zst, zfr, (const uint32_t*)nullptr,
                               (const uint32_t*)nullptr, -1, nchunks);
        }
        zsel = zst;
    }
    hipLaunchKernelGGL(lzh_zstd_decompress_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets,
                       csizes, n_total, chunk_size, out, status, 0u, stats, zsel);
#if LZH_ZSTD_STATS
    unsigned long long h[zstdd::kZClk];
    (void)hipMemcpyAsync(h, d_stats, sizeof(h), hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    unsigned long long tot = 0;
    for (int i = 0; i < zstdd::kZClk; i++) tot += h[i];
    static const char* names[zstdd::kZClk] = {"headers", "huf_table", "huf_streams", "seq_tables", "seq_decode",
                                              "emit_group", "long_seq", "tail"};
    fprintf(stderr, "zstd clocks per chunk %.0f:", (double)tot / nchunks);
    for (int i = 0; i < zstdd::kZClk; i++) fprintf(stderr, " %s %.1f%%", names[i], 100.0 * h[i] / (tot ? tot : 1));
    fprintf(stderr, "\n");
#endif
    return hipGetLastError();
}

// the sequence kernel alone, every frame in one launch on s (ragged batches: frames of up to slot_bytes)
hipError_t lzh_launch_zstd_seq(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                               uint64_t slot_bytes, uint32_t nchunks, int32_t* status, uint8_t* zt, const int32_t* zst,
                               void* zfr, hipStream_t s) {
    hipLaunchKernelGGL(lzh_zstd_seq_kernel, dim3((nchunks + zsplit::kFPW - 1) / zsplit::kFPW), dim3(64), 0, s, packed,
                       packed_readable, offsets, slot_bytes, nchunks, status, zt, zst, (zsplit::ZFrame*)zfr,
                       (unsigned long long*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, -1);
    return hipGetLastError();
}

// the sizes temp_layout.h lays a ragged batch's split-decoder temp out with (frames of up to chunk bytes)
LzhZstdSplitSizes lzh_zstd_split_sizes(uint64_t chunk, uint64_t nchunks) {
    const zsplit::ZLayout Z = zsplit::zlayout(chunk);
    return {(size_t)Z.stride, (size_t)zsplit::zdummy_bytes(nchunks), sizeof(zsplit::ZFrame),
            (size_t)(Z.bmax * sizeof(zsplit::ZHuf))};
}

// bytes of the split decoder's temp for n bytes in chunks of chunk_size (per frame: blocks, block
// positions, sequence tables, sequences; then the frame states and frame fields)
// (0 below lzh_zstd_split_min: the layout reserves two block slots (~17 KiB) and 2 x chunk of sequence
// records per frame, 20x the input at 1 KiB chunks; small frames decode in the one-wave kernel)
size_t lzh_zstd_decode_temp(uint64_t n, uint64_t chunk_size) {
    if (chunk_size < lzh_zstd_split_min) return 0;
    const uint64_t k = (n + chunk_size - 1) / chunk_size;
    const zsplit::ZLayout Z = zsplit::zlayout(chunk_size);
    return k * Z.stride + zsplit::zdummy_bytes(k) + ((k * 4 + 255) & ~255ull) + ((k * sizeof(zsplit::ZFrame) + 255) & ~255ull) + 256 +
           k * Z.bmax * sizeof(zsplit::ZHuf) + 256 + ((k * 4 + 8 + 255) & ~255ull);   // (+ the plan's frame list, counts)
}
#endif   // LZH_DEVICE_FUNCTIONS_ONLY
