// lzbench_amd/csrc/frame.h -- the LZ4 frame format as device code, for the units that write and read frames:
// frame_hip.hip (one buffer cut at a chunk size) and lz4f_ragged_hip.hip (per-chunk pointers and sizes).  Both use
// the first part: XXH32 as wave-uniform code, LZ4F_optimalBSID, the header length, the byte stores, the block
// decoder's 32-byte descriptor.  The second part is the format per frame, after a unit's own geometry: a frame's size
// from its blocks, a block's word and checksum, a frame's header words, end mark and content checksum, the decoder's
// header checks and block walk, the frame's verdict.  lz4f_ragged_hip.hip's kernels are built from it.  The kernels of
// frame_hip.hip keep the same steps as their own text for now: calling these functions there compiles to other
// machine code for all four (the profiles are keyed to their code hashes), so that move waits for a change that
// re-records them.  No kernels here.
#pragma once
#include "common.h"

namespace frm {

constexpr uint32_t P1 = 2654435761U, P2 = 2246822519U, P3 = 3266489917U, P4 = 668265263U, P5 = 374761393U;
__device__ __forceinline__ uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// XXH32 (seed 0) of bytes [0, len) of b, computed by the whole wave: lane j loads 16-byte stripe j
// of each 1 KiB batch, the four accumulators then take the stripes in order (wave-uniform code)
__device__ uint32_t xxh32_wave(const Bytes& b, uint32_t len, int lane) {
    uint32_t h;
    uint32_t p = 0;
    if (len >= 16) {
        uint32_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0u - P1;
        const uint32_t ns = len / 16;   // stripes with p < len - 15, i.e. floor(len / 16)
        for (uint32_t s0 = 0; s0 < ns; s0 += 64) {
            const uint32_t q = (s0 + (uint32_t)lane) * 16;
            const bool in = s0 + (uint32_t)lane < ns;
            const uint32_t w0 = in ? b.w32(q) : 0, w1 = in ? b.w32(q + 4) : 0, w2 = in ? b.w32(q + 8) : 0,
                           w3 = in ? b.w32(q + 12) : 0;
            const uint32_t m = min(64u, ns - s0);
            for (uint32_t j = 0; j < m; j++) {
                v1 = rotl(v1 + rdlane(w0, (int)j) * P2, 13) * P1;
                v2 = rotl(v2 + rdlane(w1, (int)j) * P2, 13) * P1;
                v3 = rotl(v3 + rdlane(w2, (int)j) * P2, 13) * P1;
                v4 = rotl(v4 + rdlane(w3, (int)j) * P2, 13) * P1;
            }
        }
        p = ns * 16;
        h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
    } else {
        h = P5;
    }
    h += len;
    const uint32_t t = b.w32((int)p), t2 = b.w32((int)p + 4), t3 = b.w32((int)p + 8), t4 = b.w32((int)p + 12);
    const uint32_t tw[4] = {uni(t), uni(t2), uni(t3), uni(t4)};
    int k = 0;
    for (; p + 4 <= len; p += 4, k++) h = rotl(h + tw[k] * P3, 17) * P4;
    for (; p < len; p++) h = rotl(h + uni(b.b((int)p)) * P5, 11) * P1;   // (bytewise: exact-size views)
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

// XXH32 (seed 0) of the n < 16 bytes held as little-endian words in hw: the short-input path (xxhash.c:383-388)
__device__ __forceinline__ uint32_t xxh32_short(const uint32_t* hw, int n) {
    uint32_t h = P5 + (uint32_t)n;
    int p = 0;
    for (; p + 4 <= n; p += 4) h = rotl(h + hw[p / 4] * P3, 17) * P4;
    for (; p < n; p++) h = rotl(h + ((hw[p / 4] >> (8 * (p & 3))) & 0xffu) * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ uint64_t bsize_of(int id) { return (uint64_t)1 << (8 + 2 * id); }

// LZ4F_optimalBSID (lz4frame.c:304-316); 0 = default = max64KB (lz4frame.c:640-641)
__device__ __forceinline__ int optimal_bsid(int req, uint64_t n) {
    int id = 4;
    uint64_t mb = 64u << 10;
    while (req > id) {
        if (n <= mb) return id;
        id++;
        mb <<= 2;
    }
    return req ? req : 4;
}

// little-endian byte stores of v at pos (a frame header field at an arbitrary byte offset)
__device__ __forceinline__ void put_le(const Bytes& o, int pos, uint64_t v, int nb) {
    for (int i = 0; i < nb; i++) o.st8(pos + i, (uint32_t)(v >> (8 * i)) & 0xffu);
}

}  // namespace frm

// LZ4F: frame header bytes for frame content size s
__device__ __forceinline__ int lz4f_header_len(int params, uint64_t s) { return 7 + (((params & 0x40) && s) ? 8 : 0); }

// Block descriptor for the block decoder: u64 source offset in packed, u64 destination offset,
// u32 stored size, u32 decoded size, u32 flags (1 = stored raw), u32 spare.
struct FrameDesc { uint64_t src, dst; uint32_t cs, ds, flags, pad; };

namespace frm {

// a frame's size from its nb blocks' sizes (bcs) and the blocks' offsets inside the frame (rel: each block's header
// word); blocks of bs bytes over a frame of s; a block is stored raw when its LZ4 block is not smaller
__device__ __forceinline__ uint64_t lz4f_frame_bytes(int params, uint64_t s, uint64_t bs, uint32_t nb, const uint32_t* bcs,
                                                     uint32_t* rel) {
    const int bcrc = (params >> 4) & 1, ccrc = (params >> 5) & 1;
    uint64_t pos = (uint64_t)lz4f_header_len(params, s);
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t bsz = (uint32_t)min(bs, s - b * bs);
        const uint32_t c = bcs[b];
        rel[b] = (uint32_t)pos;
        pos += 4 + (c >= bsz ? bsz : c) + 4 * bcrc;
    }
    return pos + 4 + 4 * ccrc;
}

// a block in its frame, after its st stored bytes were copied to dst + 4: the block word and, with cb, the block
// checksum of the stored bytes (lz4frame.c:758-761), by the workgroup's first wave
__device__ __forceinline__ void lz4f_block_edges(const Bytes& src, const Bytes& dst, uint32_t st, bool raw, int cb, int t) {
    if (t == 0) put_le(dst, 0, (uint64_t)(st | (raw ? 0x80000000u : 0u)), 4);
    if (cb && t < 64) {
        const uint32_t h = xxh32_wave(src, st, t);
        if (t == 0) put_le(dst, 4 + (int)st, h, 4);
    }
}

// a frame of fsz bytes at dst around its blocks, by one wave: the header (lz4frame.c:669-696: magic, FLG (version 01,
// independent blocks, flags), BD, content size, HC = second byte of XXH32 of FLG..content size), the end mark and the
// content checksum of the frame's input (lz4frame.c:1005-1011; src: the frame's s input bytes)
__device__ __forceinline__ void lz4f_frame_edges(int params, const Bytes& src, uint64_t s, uint64_t bs, uint32_t fsz,
                                                 const Bytes& dst, int t) {
    const int bcrc = (params >> 4) & 1, ccrc = (params >> 5) & 1, csz = (params & 0x40) && s;
    const int bsid = optimal_bsid(params & 7, s);
    const uint32_t indep = (params & 0x80) && s > bs ? 0u : 1u;   // linked blocks (frames of one block: independent)
    const uint32_t flg = (1u << 6) | (indep << 5) | ((uint32_t)bcrc << 4) | ((uint32_t)csz << 3) | ((uint32_t)ccrc << 2);
    const uint32_t bd = (uint32_t)(bsid & 7) << 4;
    uint32_t hw[3] = {flg | (bd << 8), 0, 0};   // descriptor bytes as little-endian words
    int hl = 2;
    if (csz) {
        hw[0] |= (uint32_t)(s & 0xffff) << 16;
        hw[1] = (uint32_t)(s >> 16);
        hw[2] = (uint32_t)(s >> 48);
        hl = 10;
    }
    const uint32_t h = xxh32_short(hw, hl);
    if (t == 0) {
        put_le(dst, 0, 0x184D2204u, 4);
        for (int i = 0; i < hl; i++) dst.st8(4 + i, (hw[i / 4] >> (8 * (i & 3))) & 0xffu);
        dst.st8(4 + hl, (h >> 8) & 0xffu);
        put_le(dst, (int)fsz - 4 - 4 * ccrc, 0, 4);   // end mark
    }
    if (ccrc) {
        const uint32_t c = xxh32_wave(src, (uint32_t)s, t);
        if (t == 0) put_le(dst, (int)fsz - 4, c, 4);
    }
}

// The decoder's header checks and block walk over one frame, by one wave (lz4frame.c:1150-1260 LZ4F_decodeHeader,
// :1384-1899 LZ4F_decompress): fr views the frame's cs bytes (`readable` of them may be read) at fp = packed + ioff,
// s is the size the frame must decode to, dst0 where its first byte goes.  Writes a descriptor per block to D (the
// caller zeroed the frame's slots; ceil(s / 64 KiB) of them at the least) and returns 0 or a negative status: -1
// malformed, -2 a feature outside the supported set (dictionary id, blocks that are not all full but the last).  A
// linked frame's blocks are marked so that one wave decodes them in order, each with the frame's output before it as
// its prefix (LZ4F_updateDict, lz4frame.c:1290-1306).
__device__ __forceinline__ int lz4f_parse(const Bytes& fr, const uint8_t* fp, uint64_t readable, uint64_t ioff, uint32_t cs,
                                          uint64_t s, uint64_t dst0, FrameDesc* D, int lane) {
    auto rd = [&](uint32_t p) -> uint32_t { return uni(fr.w32((int)p)); };
    int st = 0;
    const uint32_t w0 = rd(0), w1 = rd(4);
    const uint32_t flg = w1 & 0xffu, bd = (w1 >> 8) & 0xffu;
    const int bcrc = (flg >> 4) & 1, csz = (flg >> 3) & 1, ccrc = (flg >> 2) & 1, dict = flg & 1;
    const uint32_t hl = 7 + 8 * csz + 4 * dict;
    const int bid = (int)(bd >> 4) & 7;
    if (cs < 7 || w0 != 0x184D2204u || (flg >> 6) != 1 || (flg & 2) || (bd & 0x8f) || bid < 4 || cs < hl) st = -1;
    if (!st) {   // header checksum over FLG .. the optional fields
        const uint32_t hcb = (rd(hl - 1) & 0xffu);
        const uint32_t hw[4] = {rd(4), rd(8), rd(12), rd(16)};   // bytes 4 .. hl - 2 (up to 17)
        const uint32_t h = xxh32_short(hw, (int)hl - 5);
        if (hcb != ((h >> 8) & 0xffu)) st = -1;
        else if (dict) st = -2;
        else if (csz && (((uint64_t)rd(10) << 32 | rd(6)) != s)) st = -1;
    }
    const uint64_t B = bsize_of(bid);
    const uint32_t nbe = st ? 0 : (uint32_t)((s + B - 1) / B);   // blocks a full-block frame has
    uint32_t ip = hl, b = 0;
    while (!st) {
        if (ip + 4 > cs) { st = -1; break; }
        const uint32_t w = rd(ip);
        ip += 4;
        if (w == 0) break;
        const uint32_t sz = w & 0x7fffffffu;
        if (sz > B || ip + sz + 4u * (uint32_t)bcrc > cs) { st = -1; break; }
        if (b >= nbe) { st = -2; break; }
        const uint32_t ds = (uint32_t)min<uint64_t>(B, s - b * B);
        const bool raw = (w >> 31) != 0;
        if (raw && sz != ds) { st = sz > ds ? -1 : -2; break; }
        if (bcrc) {
            Bytes bb;
            bb.init_dw(fp + ip, min<uint64_t>(sz, readable > ip ? readable - ip : 0));
            const uint32_t h = xxh32_wave(bb, sz, lane);
            if (h != rd(ip + sz)) { st = -1; break; }
        }
        // flags: 1 = stored raw, 2 = a linked frame's first block (pad = the frame's block count),
        // 4 = a linked frame's later block (decoded by the first block's wave, in order)
        const uint32_t lk = (flg & 0x20) ? 0u : (b == 0 ? 2u : 4u);
        if (lane == 0) D[b] = FrameDesc{ioff + ip, dst0 + b * B, sz, ds, (raw ? 1u : 0u) | lk, 0};
        ip += sz + 4u * (uint32_t)bcrc;
        b++;
    }
    if (!st && b != nbe) st = -2;
    if (!st && !(flg & 0x20) && lane == 0) D[0].pad = b;
    if (!st && ccrc) ip += 4;
    if (!st && ip != cs) st = -1;
    return st;
}

// the verdict over a frame's maxbpf descriptor slots and the block decoder's results for them (bstat): st as it
// came from the parse, -1 a bad block, -2 a short one
__device__ __forceinline__ int blocks_verdict(int st, const FrameDesc* D, const int32_t* bstat, uint32_t maxbpf, int lane) {
    for (uint32_t b0 = 0; !st && b0 < maxbpf; b0 += 64) {
        const uint32_t b = b0 + (uint32_t)lane;
        bool badb = false, shortb = false;
        if (b < maxbpf && D[b].ds) {
            const int r = bstat[b];
            badb = r < 0 || r > (int)D[b].ds;
            shortb = r >= 0 && r < (int)D[b].ds;
        }
        if (ballot(badb)) st = -1;
        else if (ballot(shortb)) st = -2;
    }
    return st;
}

// a decoded frame's content checksum (lz4frame.c:1810-1830): fp = the frame's cs bytes, of which `readable` lie inside
// the packed buffer (a frame that ends outside it reads zeros there), out its s decoded bytes (any alignment; not
// read for s = 0); false = the frame carries one and it does not match
__device__ __forceinline__ bool lz4f_content_ok(const uint8_t* fp, uint32_t cs, uint64_t readable, const uint8_t* out,
                                                uint64_t s, int lane) {
    Bytes fr;
    fr.init(fp, min<uint64_t>(readable, 8));
    const uint32_t flg = uni(fr.w32(4)) & 0xffu;
    if (!((flg >> 2) & 1)) return true;
    Bytes o, tail;
    o.init_dw(s ? out : nullptr, s);
    const uint32_t h = xxh32_wave(o, (uint32_t)s, lane);
    tail.init(fp + cs - 4, readable >= cs ? 4 : 0);   // (bytewise: the range ends at the frame's end)
    const uint32_t c = tail.b(0) | tail.b(1) << 8 | tail.b(2) << 16 | tail.b(3) << 24;
    return h == uni(c);
}

}  // namespace frm
