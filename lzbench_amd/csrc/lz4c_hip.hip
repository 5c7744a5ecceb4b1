// lzbench_amd/csrc/lz4c_hip.hip -- LZ4 block compressor (v3) for gfx950, bit-exact with lz4 1.9.3.
//
// The uniform kernels (one buffer cut at a chunk size), their launchers and the debug exports.  The device code --
// the parse, lz4v3::compress_chunk, and the emission, lz4e -- is in lz4c.h, where the design is described.
#include "lz4c.h"

extern "C" __global__ void __launch_bounds__(64)
lzh_lz4_compress_v2_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size, int acc,
                           uint8_t* stage, uint64_t stride, uint32_t* csizes, uint32_t chunk0,
                           unsigned long long* stats) {
    // table 16 KiB | input ring 1 KiB | output ring 512 B  (17.5 KiB: 9 waves per CU)
    __shared__ __attribute__((aligned(16))) uint32_t lds[4096 + lz4v3::kRing / 4 + lz4v3::kOut / 4];
    const uint64_t chunk = (uint64_t)blockIdx.x + chunk0;
    const uint64_t off = chunk * chunk_size;
    if (off >= n_total && !(n_total == 0 && chunk == 0)) return;
    const int n = (int)min(chunk_size, n_total - off);
    const uint64_t readable = min<uint64_t>(in_readable - off, (uint64_t)n + 64);
    Bytes rin, rout;
    rin.init(in + off, readable);
    rout.init(stage + chunk * stride, stride);
    LDSA uint32_t* tab = (LDSA uint32_t*)lds;
    LDSA uint32_t* ring = tab + 4096;
    LDSA uint8_t* outb = (LDSA uint8_t*)(ring + lz4v3::kRing / 4);
    const rsrc_t nr = make_rsrc(nullptr, 0);
    if (n < 65547) {
        if (acc > 1) lz4v3::compress_chunk<true, false, false, true>(rin, n, rout, acc, tab, ring, outb, csizes + chunk, stats, nr, nullptr);
        else lz4v3::compress_chunk<true, false>(rin, n, rout, acc, tab, ring, outb, csizes + chunk, stats, nr, nullptr);
    } else {
        if (acc > 1) lz4v3::compress_chunk<false, false, false, true>(rin, n, rout, acc, tab, ring, outb, csizes + chunk, stats, nr, nullptr);
        else lz4v3::compress_chunk<false, false>(rin, n, rout, acc, tab, ring, outb, csizes + chunk, stats, nr, nullptr);
    }
}

// debug twin of the parse kernel with event counters and phase clocks (tools/lz4_stats.py)
extern "C" __global__ void __launch_bounds__(64)
lzh_lz4_compress_stats_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size, int acc,
                              uint8_t* stage, uint64_t stride, uint32_t* csizes, uint32_t chunk0,
                              unsigned long long* stats) {
    // (the parse kernel's path: records dropped by a zero-size descriptor, header into LDS scratch)
    __shared__ __attribute__((aligned(16))) uint32_t lds[4096 + lz4v3::kRing / 4 + 8];
    __shared__ uint32_t hdr[2];
    const uint64_t chunk = (uint64_t)blockIdx.x + chunk0;
    const uint64_t off = chunk * chunk_size;
    if (off >= n_total && !(n_total == 0 && chunk == 0)) return;
    const int n = (int)min(chunk_size, n_total - off);
    const uint64_t readable = min<uint64_t>(in_readable - off, (uint64_t)n + 64);
    Bytes rin, rout;
    rin.init(in + off, readable);
    rout.init(stage + chunk * stride, stride);
    LDSA uint32_t* tab = (LDSA uint32_t*)lds;
    LDSA uint32_t* ring = tab + 4096;
    const rsrc_t nr = make_rsrc(nullptr, 0);
    if (n < 65547) {
        if (acc > 1) lz4v3::compress_chunk<true, true, true, true>(rin, n, rout, acc, tab, ring, nullptr, nullptr, stats, nr, hdr);
        else lz4v3::compress_chunk<true, true, true, false>(rin, n, rout, acc, tab, ring, nullptr, nullptr, stats, nr, hdr);
    } else {
        if (acc > 1) lz4v3::compress_chunk<false, true, true, true>(rin, n, rout, acc, tab, ring, nullptr, nullptr, stats, nr, hdr);
        else lz4v3::compress_chunk<false, true, true, false>(rin, n, rout, acc, tab, ring, nullptr, nullptr, stats, nr, hdr);
    }
}

// ======================================================================= parse + emit split
// The parse kernel (one wave per chunk, the compress_chunk loop of lz4c.h with kRec) leaves every
// sequence as an 8-byte record; lzh_lz4_emit_kernel, which needs no hash table and runs at high
// occupancy, lays the LZ4 block out (lz4.c:1022-1135 sequence format, :1204-1231 last literals):
// for 64 records at a time a wave computes input anchors and output offsets by prefix sums,
// every lane writes its sequence's bytes into an LDS ring, and the ring leaves for the staging
// slot as aligned dwords.  Chunks up to 16 MiB (24-bit literal / match-length fields).

extern "C" __global__ void __launch_bounds__(64)
lzh_lz4_parse_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size, int acc,
                     uint8_t* recs, uint64_t rec_stride, uint32_t* rec_hdr, uint64_t frame_size, uint32_t bpf) {
    // table only (the P sides from a register window, compress_chunk's kRec)
    __shared__ __attribute__((aligned(16))) uint32_t lds[4096];
    const uint64_t chunk = blockIdx.x;
    uint64_t off;
    int n;
    if (!block_span(chunk, n_total, chunk_size, frame_size, bpf, off, n)) return;
    const uint64_t readable = min<uint64_t>(in_readable - off, (uint64_t)n + 64);
#include "lz4c_parse_body.inc"
}

extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LZH_EMIT_WAVES, 8)))
lzh_lz4_emit_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size,
                    const uint8_t* recs, uint64_t rec_stride, const uint32_t* rec_hdr, uint8_t* stage, uint64_t stride,
                    uint32_t* csizes, uint64_t frame_size, uint32_t bpf) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[lz4e::kRingB];
    __shared__ __attribute__((aligned(16))) uint32_t ibuf[lz4e::kSpan / 4 + 4];   // input span of a group
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    uint64_t off;
    int n;
    if (!block_span(chunk, n_total, chunk_size, frame_size, bpf, off, n)) return;
    Bytes in_b;
    in_b.init(in + off, min<uint64_t>(in_readable - off, (uint64_t)n + 64));
#include "lz4c_emit_body.inc"
}

#ifndef LZH_NO_LINKED_KERNEL
// LZ4 frames with linked blocks (LZ4F_blockLinked, the LZ4F default; lz4frame.c:651-655, :777-782):
// one wave per frame walks its blocks in order with one byU32 table, as LZ4_compress_fast_continue
// does over a stable source (lz4.c:1565-1628, prefix mode).  Each block is compressed with the
// limitedOutput budget size - 1 (LZ4F_makeBlock, lz4frame.c:740-763); a block that does not fit is
// stored raw (bcs = its size) and its table is rebuilt as the reference leaves it at the failing
// check: the table is saved to `snap` (16 KiB per frame) before every block and a failed block is
// replayed from it up to the failing probe.  A frame of one block is independent (lz4frame.c:394-395)
// and goes through the chunk codec.  Block i of frame f: staging slot f * bpf + b, size bcs[i].
template <bool kFast>
__device__ void lz4f_linked_frame(const Bytes& rin, uint64_t s, uint64_t bs, uint32_t bpf, uint64_t f, int acc,
                                  uint8_t* stage, uint64_t stride, uint32_t* bcs, uint32_t* snap, LDSA uint32_t* tab,
                                  LDSA uint32_t* ring, LDSA uint8_t* outb) {
    const int lane = threadIdx.x;
    const rsrc_t nr = make_rsrc(nullptr, 0);
    const uint32_t nb = (uint32_t)((s + bs - 1) / bs);
    const rsrc_t sn = make_rsrc(snap + f * 4096, 16384);
    for (uint32_t b = 0; b < nb; b++) {
        const int b0 = (int)(b * bs), bn = (int)min<uint64_t>(bs, s - b * bs);
        const uint64_t i = f * bpf + b;
        if (b > 0) {   // the table before this block (a failed block replays from it)
            wave_lds_fence();
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int d = 4 * (k * LZH_WAVE + lane);
                const u32x4 v = {tab[d], tab[d + 1], tab[d + 2], tab[d + 3]};
                __builtin_amdgcn_raw_buffer_store_b128(v, sn, 4 * d, 0, 0);
            }
        }
        Bytes rout;
        rout.init(stage + i * stride, stride);
        lz4v3::LinkCtl L{b0, bn - 1, -1, b > 0, -1};
        lz4v3::compress_chunk<false, false, false, kFast, true>(rin, bn, rout, acc, tab, ring, outb, bcs + i,
                                                                        nullptr, nr, nullptr, &L);
        if (L.abort >= 0) {   // replay up to the failing probe: the table the next block starts from
            if (b > 0) {
                wait_vm();
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int d = 4 * (k * LZH_WAVE + lane);
                    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(sn, 4 * d, 0, 0);
                    tab[d] = v[0]; tab[d + 1] = v[1]; tab[d + 2] = v[2]; tab[d + 3] = v[3];
                }
                wave_lds_fence();
            }
            Bytes nul;
            nul.r = nr;
            nul.sh = 0;
            lz4v3::LinkCtl Rp{b0, 0x7fffffff, L.abort, b > 0, -1};
            lz4v3::compress_chunk<false, false, false, kFast, true>(rin, bn, nul, acc, tab, ring, outb, nullptr,
                                                                            nullptr, nr, nullptr, &Rp);
        }
        wave_lds_fence();
    }
}

extern "C" __global__ void __launch_bounds__(64)
lzh_lz4f_linked_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t fs, uint64_t bs, uint32_t bpf,
                       int acc, uint8_t* stage, uint64_t stride, uint32_t* bcs, uint32_t* snap) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[4096 + lz4v3::kRing / 4 + lz4v3::kOut / 4];
    const uint64_t f = blockIdx.x;
    const uint64_t foff = f * fs;
    if (foff >= n_total) return;
    const uint64_t s = min(fs, n_total - foff);
    Bytes rin;
    rin.init(in + foff, min<uint64_t>(in_readable - foff, s + 64));
    LDSA uint32_t* tab = (LDSA uint32_t*)lds;
    LDSA uint32_t* ring = tab + 4096;
    LDSA uint8_t* outb = (LDSA uint8_t*)(ring + lz4v3::kRing / 4);
    if (s <= bs) {   // one block: independent (the chunk codec with its own table type)
        const rsrc_t nr = make_rsrc(nullptr, 0);
        Bytes rout;
        rout.init(stage + f * bpf * stride, stride);
        uint32_t* cs = bcs + f * bpf;
        const int n = (int)s;
        if (n < 65547) {
            if (acc > 1) lz4v3::compress_chunk<true, false, false, true>(rin, n, rout, acc, tab, ring, outb, cs, nullptr, nr, nullptr);
            else lz4v3::compress_chunk<true, false>(rin, n, rout, acc, tab, ring, outb, cs, nullptr, nr, nullptr);
        } else {
            if (acc > 1) lz4v3::compress_chunk<false, false, false, true>(rin, n, rout, acc, tab, ring, outb, cs, nullptr, nr, nullptr);
            else lz4v3::compress_chunk<false, false>(rin, n, rout, acc, tab, ring, outb, cs, nullptr, nr, nullptr);
        }
        return;
    }
    if (acc > 1) lz4f_linked_frame<true>(rin, s, bs, bpf, f, acc, stage, stride, bcs, snap, tab, ring, outb);
    else lz4f_linked_frame<false>(rin, s, bs, bpf, f, acc, stage, stride, bcs, snap, tab, ring, outb);
}

#endif
#include "../../include/lzbench_hip.h"
#include "launch.h"
size_t lzh_lz4_rec_stride(uint64_t chunk_size) { return ((chunk_size / 4 + 4) * 8 + 255) / 256 * 256; }

hipError_t lzh_launch_lz4_compress_v2(const LzhInput& I, int acc, const LzhSlots& S, uint32_t* csizes, hipStream_t s) {
    if (I.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_lz4_compress_v2_kernel, dim3(I.nchunks), dim3(64), 0, s, I.in, I.n_total, I.in_readable,
                       I.chunk_size, acc, S.stage, S.stride, csizes, 0u, (unsigned long long*)nullptr);
    return hipGetLastError();
}

// parse kernel + emit kernel (records in S.recs: nchunks x S.rec_stride bytes; 8 bytes per chunk at S.hdr);
// stage_mask bit 0 = parse, bit 1 = emit (profiling runs one of them)
hipError_t lzh_launch_lz4_split(const LzhInput& I, int acc, const LzhSlots& S, uint32_t* csizes, int stage_mask,
                                hipStream_t s) {
    if (I.nchunks == 0) return hipSuccess;
    const bool framed = I.bpf > 1;
    const uint64_t frame_size = framed ? I.frame_size : I.chunk_size;
    const uint32_t bpf = framed ? I.bpf : 1;
    if (stage_mask & 1)
        hipLaunchKernelGGL(lzh_lz4_parse_kernel, dim3(I.nchunks), dim3(64), 0, s, I.in, I.n_total, I.in_readable,
                           I.chunk_size, acc, S.recs, S.rec_stride, S.hdr, frame_size, bpf);
    if (stage_mask & 2)
        hipLaunchKernelGGL(lzh_lz4_emit_kernel, dim3(I.nchunks), dim3(64), 0, s, I.in, I.n_total, I.in_readable,
                           I.chunk_size, (const uint8_t*)S.recs, S.rec_stride, (const uint32_t*)S.hdr, S.stage, S.stride,
                           csizes, frame_size, bpf);
    return hipGetLastError();
}

hipError_t lzh_launch_lz4f_linked(const LzhInput& I, int acc, const LzhFrameSlots& F, hipStream_t s) {
    if (I.nframes == 0) return hipSuccess;
#ifdef LZH_NO_LINKED_KERNEL
    return hipErrorNotSupported;
#else
    hipLaunchKernelGGL(lzh_lz4f_linked_kernel, dim3(I.nframes), dim3(64), 0, s, I.in, I.n_total, I.in_readable,
                       I.frame_size, I.chunk_size, I.bpf, acc, F.blocks.stage, F.blocks.stride, F.bcs,
                       (uint32_t*)F.blocks.recs);
    return hipGetLastError();
#endif
}

// debug: run the v2 kernel with event counters (16 x u64 device buffer)
extern "C" int lzh_debug_lz4_stats(const void* d_in, uint64_t n, uint64_t in_readable, uint64_t chunk_size, int acc,
                                   void* d_stage, uint32_t* d_csizes, unsigned long long* d_stats, void* stream) {
    const uint64_t k = (n + chunk_size - 1) / chunk_size;
    const uint64_t stride = lzh_stage_stride(LZH_CODEC_LZ4, chunk_size);
    hipLaunchKernelGGL(lzh_lz4_compress_stats_kernel, dim3((unsigned)k), dim3(64), 0, (hipStream_t)stream,
                       (const uint8_t*)d_in, n, in_readable, chunk_size, acc, (uint8_t*)d_stage, stride, d_csizes, 0u,
                       d_stats);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
