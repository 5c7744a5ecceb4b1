// lzbench_amd/csrc/snappyc_hip.hip -- snappy raw compressor for gfx950, bit-exact with snappy
// 1.1.8 (reference snappy/snappy.cc:510-681, framing :1043-1111).
//
// The uniform kernels (one buffer cut at a chunk size), their launchers and the debug exports.  The device code --
// the parse, snv2::compress_fragment, and the emission, sne -- is in snappyc.h, where the design is described.
#include "snappyc.h"

extern "C" __global__ void __launch_bounds__(64)
lzh_snappy_compress_v2_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size,
                              uint8_t* stage, uint64_t stride, uint32_t* csizes, uint32_t chunk0,
                              unsigned long long* stats) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[(1 << 13) + 256 + LZH_WAVE / 4];   // table | ring | marks
    const int lane = threadIdx.x;
    const uint64_t chunk = (uint64_t)blockIdx.x + chunk0;
    const uint64_t off = chunk * chunk_size;
    if (off >= n_total && !(n_total == 0 && chunk == 0)) return;
    const uint32_t n = (uint32_t)min(chunk_size, n_total - off);
    Bytes rout;
    rout.init(stage + chunk * stride, stride);
    int op = 0;
    {   // varint32 uncompressed length (snappy.cc:1047-1050)
        uint32_t v = n;
        int nb = 1;
        while (v >= 128) { v >>= 7; nb++; }
        if (lane < nb) rout.st8(lane, ((n >> (7 * lane)) & 0x7fu) | (lane + 1 < nb ? 0x80u : 0u));
        op = nb;
    }
    for (uint32_t fpos = 0; fpos < n; fpos += 65536u) {
        const int fn = (int)min(65536u, n - fpos);
        const uint64_t readable = min<uint64_t>(in_readable - off - fpos, (uint64_t)fn + 64);
        Bytes rin;
        rin.init(in + off + fpos, readable);
        int nrec = 0;
        op = snv2::compress_fragment<false>(rin, fn, rout, op, (LDSA uint16_t*)lds, (LDSA uint32_t*)lds + (1 << 13),
                                            (LDSA uint8_t*)((LDSA uint32_t*)lds + (1 << 13) + 256), stats,
                                            make_rsrc(nullptr, 0), nrec, 0);
    }
    if (lane == 0) csizes[chunk] = (uint32_t)op;
}

// ======================================================================= parse + emit split
// As for LZ4 (lz4c_hip.hip): the parse kernel (the loop of snappyc.h with kRec, no output marks) leaves
// 8-byte records; lzh_snappy_emit_kernel (no hash table: high occupancy) writes the varint header
// (snappy.cc:1047-1050) and lays out EmitLiteral / EmitCopy (:342-443) for 64 records at a time.

extern "C" __global__ void __launch_bounds__(64)
lzh_snappy_parse_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size,
                        uint8_t* recs, uint64_t rec_stride, uint32_t* rec_hdr, uint32_t frags) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[(1 << 13) + 256 + 8];   // table | ring + mirror
    const uint64_t chunk = blockIdx.x / frags;
    const uint32_t f = blockIdx.x - (uint32_t)chunk * frags;
    const uint64_t off = chunk * chunk_size;
    if (off >= n_total && !(n_total == 0 && chunk == 0)) return;
    const uint32_t n = (uint32_t)min(chunk_size, n_total - off);
#include "snappyc_parse_body.inc"
}

// -b64 and smaller chunks: a single fragment, one wave
extern "C" __global__ void __launch_bounds__(64)
lzh_snappy_emit_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size,
                       const uint8_t* recs, uint64_t rec_stride, const uint32_t* rec_hdr, uint8_t* stage,
                       uint64_t stride, uint32_t* csizes, uint32_t frags) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[sne::kRingB];
    __shared__ __attribute__((aligned(16))) uint32_t ibuf[sne::kSpanDw];
    sne::emit_chunk<false>((LDSA uint8_t*)ring, (LDSA uint32_t*)ibuf, nullptr, in, n_total, in_readable, chunk_size,
                           recs, rec_stride, rec_hdr, stage, stride, csizes, frags);
}

// larger chunks: kW >= min(fragments, 8) waves (the block has exactly that many), each with its
// ring and span, and the fragment sizes
template <int kW>
__global__ void __launch_bounds__(64 * kW)
lzh_snappy_emit_frag_kernel(const uint8_t* in, uint64_t n_total, uint64_t in_readable, uint64_t chunk_size,
                            const uint8_t* recs, uint64_t rec_stride, const uint32_t* rec_hdr, uint8_t* stage,
                            uint64_t stride, uint32_t* csizes, uint32_t frags) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kW * sne::kRingB];
    __shared__ __attribute__((aligned(16))) uint32_t ibuf[kW * sne::kSpanDw];
    __shared__ uint32_t fsz[sne::kMaxFrags];
    sne::emit_chunk<true>((LDSA uint8_t*)ring, (LDSA uint32_t*)ibuf, (LDSA uint32_t*)fsz, in, n_total, in_readable,
                          chunk_size, recs, rec_stride, rec_hdr, stage, stride, csizes, frags);
}

#include "launch.h"
uint32_t lzh_snappy_frags(uint64_t chunk_size) { return (uint32_t)((chunk_size + 65535) >> 16); }
size_t lzh_snappy_rec_stride(uint64_t chunk_size) {
    const uint32_t frags = lzh_snappy_frags(chunk_size);
    if (frags > 1) return (size_t)frags * kFragRecs * 8;   // (kFragRecs * 8 is a multiple of 256)
    return ((chunk_size / 4 + 8) * 8 + 255) / 256 * 256;
}

// parse kernel + emit kernel (records in S.recs: nchunks x S.rec_stride bytes; a u32 count per fragment at S.hdr);
// stage_mask bit 0 = parse, bit 1 = emit
hipError_t lzh_launch_snappy_split(const LzhInput& I, const LzhSlots& S, uint32_t* csizes, int stage_mask, hipStream_t s) {
    if (I.nchunks == 0) return hipSuccess;
    const uint32_t frags = lzh_snappy_frags(I.chunk_size);
    if (stage_mask & 1)
        hipLaunchKernelGGL(lzh_snappy_parse_kernel, dim3(I.nchunks * frags), dim3(64), 0, s, I.in, I.n_total,
                           I.in_readable, I.chunk_size, S.recs, S.rec_stride, S.hdr, frags);
    if (stage_mask & 2) {
        if (frags > (uint32_t)sne::kMaxFrags) return hipErrorInvalidValue;
        lzh_launch_snappy_emit(lzh_snappy_emit_kernel, lzh_snappy_emit_frag_kernel<2>, lzh_snappy_emit_frag_kernel<4>,
                               lzh_snappy_emit_frag_kernel<8>, frags, I.nchunks, s, I.in, I.n_total, I.in_readable,
                               I.chunk_size, S.recs, S.rec_stride, S.hdr, S.stage, S.stride, csizes, frags);
    }
    return hipGetLastError();
}

hipError_t lzh_launch_snappy_compress_v2(const LzhInput& I, const LzhSlots& S, uint32_t* csizes, hipStream_t s) {
    if (I.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_snappy_compress_v2_kernel, dim3(I.nchunks), dim3(64), 0, s, I.in, I.n_total, I.in_readable,
                       I.chunk_size, S.stage, S.stride, csizes, 0u, (unsigned long long*)nullptr);
    return hipGetLastError();
}

#ifdef LZH_SN_CLK
extern "C" int lzh_debug_snappy_clocks(unsigned long long* host, int reset) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(snv2::lzh_sn_clk_buf), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(snv2::lzh_sn_clk_buf), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
