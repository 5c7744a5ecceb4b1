// lzbench_amd/csrc/ragged_hip.hip -- ragged batches on the device API (include/lzbench_hip.h 3b): the chunks
// of a batch are given by device arrays of pointers and sizes instead of one buffer cut at a chunk size.
//
// The entry points here are the parse, emit and pack kernels of lz4c_hip.hip, snappyc_hip.hip and
// pack_hip.hip with another chunk lookup: ragged_span (common.h) loads chunk blockIdx.x's pointer and size
// once and makes them wave-uniform, and the kernel body that follows is the uniform kernel's, shared as
// text (the *_body.inc files) under the names the uniform kernels use: in + off is the chunk's address
// (off = 0 here), in_readable - off the bytes that may be read from it (n + 16 here), n its size.
// The two codecs' device functions come from their headers (lz4c.h, snappyc.h), so every function has the
// one caller per code object that it has in its codec's own unit and is inlined as it is there.  Nothing
// here changes the uniform kernels' code (profiles/traffic*.json are keyed to their code hashes).
//
// Every slot (staging, records) is sized for the batch's max_bytes and reached through a buffer
// descriptor of that size.  A chunk whose device-side size passes max_bytes is not processed: no kernel
// touches its slots, its compressed size is 0.  Decoding reuses the block decoder's 32-byte descriptors
// (decode_hip.hip decompress_chunk): lzh_ragged_desc_kernel fills one per chunk with the chunk's
// absolute output address as the destination offset.
#include "lz4c.h"
#include "snappyc.h"

// ----------------------------------------------------------------------------------------- LZ4
extern "C" __global__ void __launch_bounds__(64)
lzh_lz4_parse_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int acc,
                            uint8_t* recs, uint64_t rec_stride, uint32_t* rec_hdr) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[4096];   // table only
    const uint64_t chunk = blockIdx.x;
    const uint64_t off = 0;
    const uint8_t* in;
    int n;
    if (!ragged_span(in_ptrs, in_bytes, chunk, max_bytes, in, n)) return;
    const uint64_t readable = (uint64_t)n + 16;
#include "lz4c_parse_body.inc"
}

extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LZH_EMIT_WAVES, 8)))
lzh_lz4_emit_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes,
                           const uint8_t* recs, uint64_t rec_stride, const uint32_t* rec_hdr, uint8_t* stage,
                           uint64_t stride, uint32_t* csizes) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[lz4e::kRingB];
    __shared__ __attribute__((aligned(16))) uint32_t ibuf[lz4e::kSpan / 4 + 4];   // input span of a group
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint8_t* in;
    int n;
    if (!ragged_span(in_ptrs, in_bytes, chunk, max_bytes, in, n)) {
        if (lane == 0) csizes[chunk] = 0;
        return;
    }
    Bytes in_b;
    in_b.init(in, (uint64_t)n + 16);
#include "lz4c_emit_body.inc"
}

// -------------------------------------------------------------------------------------- snappy
// (grid: chunks x frags, frags = the fragments of max_bytes; a chunk's fragments past its end only write
// their record count)
extern "C" __global__ void __launch_bounds__(64)
lzh_snappy_parse_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, uint8_t* recs,
                               uint64_t rec_stride, uint32_t* rec_hdr, uint32_t frags) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[(1 << 13) + 256 + 8];   // table | ring + mirror
    const uint64_t chunk = blockIdx.x / frags;
    const uint32_t f = blockIdx.x - (uint32_t)chunk * frags;
    const uint64_t off = 0;
    const uint8_t* in;
    int sn;
    if (!ragged_span(in_ptrs, in_bytes, chunk, max_bytes, in, sn)) return;
    const uint32_t n = (uint32_t)sn;
    const uint64_t in_readable = (uint64_t)n + 16;
#include "snappyc_parse_body.inc"
}

namespace sne {
template <bool kMulti>
__device__ __forceinline__ void emit_ragged(LDSA uint8_t* rings, LDSA uint32_t* ibufs, LDSA uint32_t* fsz,
                                            const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes,
                                            const uint8_t* recs, uint64_t rec_stride, const uint32_t* rec_hdr,
                                            uint8_t* stage, uint64_t stride, uint32_t* csizes, uint32_t frags) {
    const int lane = threadIdx.x & 63, wave = kMulti ? threadIdx.x >> 6 : 0, W = kMulti ? blockDim.x >> 6 : 1;
    const uint64_t chunk = blockIdx.x;
    const uint64_t off = 0;
    const uint8_t* in;
    int sn;
    if (!ragged_span(in_ptrs, in_bytes, chunk, max_bytes, in, sn)) {   // (the whole workgroup: one chunk each)
        if (threadIdx.x == 0) csizes[chunk] = 0;
        return;
    }
    const uint32_t n = (uint32_t)sn;
    const uint64_t in_readable = (uint64_t)n + 16;
#include "snappyc_emit_body.inc"
}
}  // namespace sne

// max_bytes up to 64 KiB: a single fragment, one wave
extern "C" __global__ void __launch_bounds__(64)
lzh_snappy_emit_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes,
                              const uint8_t* recs, uint64_t rec_stride, const uint32_t* rec_hdr, uint8_t* stage,
                              uint64_t stride, uint32_t* csizes, uint32_t frags) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[sne::kRingB];
    __shared__ __attribute__((aligned(16))) uint32_t ibuf[sne::kSpanDw];
    sne::emit_ragged<false>((LDSA uint8_t*)ring, (LDSA uint32_t*)ibuf, nullptr, in_ptrs, in_bytes, max_bytes, recs,
                            rec_stride, rec_hdr, stage, stride, csizes, frags);
}

// larger max_bytes: kW >= min(frags, 8) waves, each with its ring and span, and the fragment sizes
template <int kW>
__global__ void __launch_bounds__(64 * kW)
lzh_snappy_emit_frag_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes,
                                   const uint8_t* recs, uint64_t rec_stride, const uint32_t* rec_hdr, uint8_t* stage,
                                   uint64_t stride, uint32_t* csizes, uint32_t frags) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kW * sne::kRingB];
    __shared__ __attribute__((aligned(16))) uint32_t ibuf[kW * sne::kSpanDw];
    __shared__ uint32_t fsz[sne::kMaxFrags];
    sne::emit_ragged<true>((LDSA uint8_t*)ring, (LDSA uint32_t*)ibuf, (LDSA uint32_t*)fsz, in_ptrs, in_bytes, max_bytes,
                           recs, rec_stride, rec_hdr, stage, stride, csizes, frags);
}

// ---------------------------------------------------------------------------------------- pack
// (a chunk larger than max_bytes has csizes[c] = 0 and packs nothing)
extern "C" __global__ void __launch_bounds__(256)
lzh_pack_ragged_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, const uint8_t* stage,
                       uint64_t stride, const uint32_t* csizes, const uint64_t* offsets, uint8_t* packed,
                       uint64_t packed_cap) {
    const uint64_t c = blockIdx.x;
    const uint64_t ioff = 0;
    const uint8_t* in;
    int sn;
    if (!ragged_span(in_ptrs, in_bytes, c, max_bytes, in, sn)) return;
    const uint32_t part = (uint32_t)sn;
    const uint64_t in_readable = (uint64_t)part + 16;
#include "pack_body.inc"
}

// -------------------------------------------------------------------------------------- decode
// descriptor i (frame_hip.hip FrameDesc): source offset in packed, destination = the chunk's address (the block
// decoder is launched with a null output base), stored and decoded size, flags 1 = stored raw, 16 = skip
extern "C" __global__ void __launch_bounds__(256)
lzh_ragged_desc_kernel(const uint64_t* offsets, const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                       uint64_t max_bytes, uint32_t* desc, int32_t* status, uint32_t nchunks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchunks) return;
    const uint64_t src = offsets[i], dst = (uint64_t)out_ptrs[i], ob = out_bytes[i];
    const uint32_t cs = csizes[i];
    const bool over = ob > max_bytes;
    const u32x4 lo = {(uint32_t)src, (uint32_t)(src >> 32), (uint32_t)dst, (uint32_t)(dst >> 32)};
    const u32x4 hi = {cs, over ? 0u : (uint32_t)ob, over ? 16u : (cs == ob ? 1u : 0u), 0u};
    ((u32x4*)desc)[2 * (uint64_t)i] = lo;
    ((u32x4*)desc)[2 * (uint64_t)i + 1] = hi;
    if (over) status[i] = -1;
}

#include <algorithm>
#include "launch.h"

hipError_t lzh_launch_lz4_ragged(const LzhBatch& B, int acc, const LzhSlots& S, uint32_t* csizes, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_lz4_parse_ragged_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes, B.max_bytes, acc,
                       S.recs, S.rec_stride, S.hdr);
    hipLaunchKernelGGL(lzh_lz4_emit_ragged_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes, B.max_bytes,
                       (const uint8_t*)S.recs, S.rec_stride, (const uint32_t*)S.hdr, S.stage, S.stride, csizes);
    return hipGetLastError();
}

uint32_t lzh_snappy_ragged_frags(uint64_t max_bytes) { return std::max(1u, lzh_snappy_frags(max_bytes)); }

hipError_t lzh_launch_snappy_ragged(const LzhBatch& B, const LzhSlots& S, uint32_t* csizes, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    const uint32_t frags = lzh_snappy_ragged_frags(B.max_bytes);
    if (frags > (uint32_t)sne::kMaxFrags || (uint64_t)B.nchunks * frags > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lzh_snappy_parse_ragged_kernel, dim3(B.nchunks * frags), dim3(64), 0, s, B.ptrs, B.bytes,
                       B.max_bytes, S.recs, S.rec_stride, S.hdr, frags);
    lzh_launch_snappy_emit(lzh_snappy_emit_ragged_kernel, lzh_snappy_emit_frag_ragged_kernel<2>,
                           lzh_snappy_emit_frag_ragged_kernel<4>, lzh_snappy_emit_frag_ragged_kernel<8>, frags, B.nchunks,
                           s, B.ptrs, B.bytes, B.max_bytes, S.recs, S.rec_stride, S.hdr, S.stage, S.stride, csizes, frags);
    return hipGetLastError();
}

hipError_t lzh_launch_pack_ragged(const LzhBatch& B, const LzhSlots& S, const uint32_t* csizes, const uint64_t* offsets,
                                  uint8_t* packed, uint64_t packed_cap, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_pack_ragged_kernel, dim3(B.nchunks), dim3(256), 0, s, B.ptrs, B.bytes, B.max_bytes,
                       (const uint8_t*)S.stage, S.stride, csizes, offsets, packed, packed_cap);
    return hipGetLastError();
}

hipError_t lzh_launch_ragged_desc(const uint64_t* offsets, const uint32_t* csizes, void* const* out_ptrs,
                                  const uint64_t* out_bytes, uint64_t max_bytes, void* desc, int32_t* status,
                                  uint32_t nchunks, hipStream_t s) {
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_ragged_desc_kernel, dim3((nchunks + 255) / 256), dim3(256), 0, s, offsets, csizes, out_ptrs,
                       out_bytes, max_bytes, (uint32_t*)desc, status, nchunks);
    return hipGetLastError();
}
