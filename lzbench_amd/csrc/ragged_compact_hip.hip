// lzbench_amd/csrc/ragged_compact_hip.hip -- the compact compress layout of ragged batches (include/lzbench_hip.h
// 3b, lzh_compress_ragged_compact_async): the entry points of ragged_hip.hip with every chunk's staging slot and
// record slot sized from the chunk's own size (ragged_slots.h) and placed by an exclusive scan, so a batch's temp
// grows with its total bytes and not with nchunks x its largest chunk.
//
//   lzh_compact_slots_kernel   chunk i's two slot sizes (u32; 0 for a chunk over max_bytes)
//   lzh_launch_scan (twice)    the slots' offsets inside the staging region and the record region
//   parse / emit / pack        as in ragged_hip.hip, slots reached through those offsets and sizes
//
// A chunk is processed exactly when its size is at most max_bytes and both of its slots end inside their
// regions (compact_span, ragged_slots.h; the host sizes the regions for the promised total, api.cpp).  Any other chunk is
// handled as an oversize chunk of ragged_hip.hip: csizes[i] = 0, no packed bytes, no kernel touches a slot.
//
// The kernel bodies are the uniform kernels' text (*_body.inc), which names a slot `recs + chunk * rec_stride`
// of `(uint32_t)rec_stride` bytes (and `stage + chunk * stride`).  That text stays as it is -- moving the
// expression changes the uniform kernels' schedule and with it their code hashes -- so here rec_stride and
// stride are CompactSlot values (ragged_slots.h): chunk * slot is the slot's scanned offset, an explicit cast of it to an integer
// type the slot's own size (the two forms the bodies use; nothing else compiles).  The buffer descriptors the bodies build are therefore bounded by the chunk's own slot.
// As in ragged_hip.hip the two codecs' device functions come from their headers.
#include "lz4c.h"
#include "snappyc.h"
#include "launch.h"
#include "ragged_slots.h"

static_assert(kLzhSnFragRecBytes == (uint64_t)kFragRecs * 8, "ragged_slots.h: the snappy fragment's record stride");

// -------------------------------------------------------------------------------------- slot sizes
extern "C" __global__ void __launch_bounds__(256)
lzh_compact_slots_kernel(const uint64_t* in_bytes, uint64_t max_bytes, int codec, uint32_t* stage_sz, uint32_t* rec_sz,
                         uint32_t nchunks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchunks) return;
    const uint64_t b = in_bytes[i];
    const bool over = b > max_bytes;
    stage_sz[i] = over ? 0u : (uint32_t)lzh_slot_stage_bytes(codec, b);
    rec_sz[i] = over ? 0u : (uint32_t)lzh_slot_rec_bytes(codec, b, max_bytes > 65536);
}

// ----------------------------------------------------------------------------------------- LZ4
extern "C" __global__ void __launch_bounds__(64)
lzh_lz4_parse_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, int acc,
                             uint8_t* recs, uint32_t* rec_hdr, const LzhCompactLayout L) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[4096];   // table only
    const uint64_t chunk = blockIdx.x;
    const uint64_t off = 0;
    const uint8_t* in;
    int n;
    CompactSlot stride, rec_stride;
    if (!compact_span(in_ptrs, in_bytes, chunk, max_bytes, L, in, n, stride, rec_stride)) return;
    const uint64_t readable = (uint64_t)n + 16;
#include "lz4c_parse_body.inc"
}

extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LZH_EMIT_WAVES, 8)))
lzh_lz4_emit_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes,
                            const uint8_t* recs, const uint32_t* rec_hdr, uint8_t* stage, uint32_t* csizes,
                            const LzhCompactLayout L) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[lz4e::kRingB];
    __shared__ __attribute__((aligned(16))) uint32_t ibuf[lz4e::kSpan / 4 + 4];   // input span of a group
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint8_t* in;
    int n;
    CompactSlot stride, rec_stride;
    if (!compact_span(in_ptrs, in_bytes, chunk, max_bytes, L, in, n, stride, rec_stride)) {
        if (lane == 0) csizes[chunk] = 0;
        return;
    }
    Bytes in_b;
    in_b.init(in, (uint64_t)n + 16);
#include "lz4c_emit_body.inc"
}

// -------------------------------------------------------------------------------------- snappy
// (grid: chunks x frags, frags = the fragments of max_bytes; with frags > 1 every chunk, however small, keeps
// fragment f's records at record f * kFragRecs of its slot: lzh_slot_rec_bytes' multi layout)
extern "C" __global__ void __launch_bounds__(64)
lzh_snappy_parse_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, uint8_t* recs,
                                uint32_t* rec_hdr, uint32_t frags, const LzhCompactLayout L) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[(1 << 13) + 256 + 8];   // table | ring + mirror
    const uint64_t chunk = blockIdx.x / frags;
    const uint32_t f = blockIdx.x - (uint32_t)chunk * frags;
    const uint64_t off = 0;
    const uint8_t* in;
    int sn;
    CompactSlot stride, rec_stride;
    if (!compact_span(in_ptrs, in_bytes, chunk, max_bytes, L, in, sn, stride, rec_stride)) return;
    const uint32_t n = (uint32_t)sn;
    const uint64_t in_readable = (uint64_t)n + 16;
#include "snappyc_parse_body.inc"
}

namespace sne {
template <bool kMulti>
__device__ __forceinline__ void emit_compact(LDSA uint8_t* rings, LDSA uint32_t* ibufs, LDSA uint32_t* fsz,
                                             const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes,
                                             const uint8_t* recs, const uint32_t* rec_hdr, uint8_t* stage,
                                             uint32_t* csizes, uint32_t frags, const LzhCompactLayout& L) {
    const int lane = threadIdx.x & 63, wave = kMulti ? threadIdx.x >> 6 : 0, W = kMulti ? blockDim.x >> 6 : 1;
    const uint64_t chunk = blockIdx.x;
    const uint64_t off = 0;
    const uint8_t* in;
    int sn;
    CompactSlot stride, rec_stride;
    if (!compact_span(in_ptrs, in_bytes, chunk, max_bytes, L, in, sn, stride, rec_stride)) {   // (the whole workgroup)
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
lzh_snappy_emit_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes,
                               const uint8_t* recs, const uint32_t* rec_hdr, uint8_t* stage, uint32_t* csizes,
                               uint32_t frags, const LzhCompactLayout L) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[sne::kRingB];
    __shared__ __attribute__((aligned(16))) uint32_t ibuf[sne::kSpanDw];
    sne::emit_compact<false>((LDSA uint8_t*)ring, (LDSA uint32_t*)ibuf, nullptr, in_ptrs, in_bytes, max_bytes, recs,
                             rec_hdr, stage, csizes, frags, L);
}

// larger max_bytes: kW >= min(frags, 8) waves, each with its ring and span, and the fragment sizes
template <int kW>
__global__ void __launch_bounds__(64 * kW)
lzh_snappy_emit_frag_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes,
                                    const uint8_t* recs, const uint32_t* rec_hdr, uint8_t* stage, uint32_t* csizes,
                                    uint32_t frags, const LzhCompactLayout L) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kW * sne::kRingB];
    __shared__ __attribute__((aligned(16))) uint32_t ibuf[kW * sne::kSpanDw];
    __shared__ uint32_t fsz[sne::kMaxFrags];
    sne::emit_compact<true>((LDSA uint8_t*)ring, (LDSA uint32_t*)ibuf, (LDSA uint32_t*)fsz, in_ptrs, in_bytes, max_bytes,
                            recs, rec_hdr, stage, csizes, frags, L);
}

// ---------------------------------------------------------------------------------------- pack
// (a chunk that was not processed has csizes[c] = 0 and packs nothing)
extern "C" __global__ void __launch_bounds__(256)
lzh_pack_compact_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, const uint8_t* stage,
                        const uint32_t* csizes, const uint64_t* offsets, uint8_t* packed, uint64_t packed_cap,
                        const LzhCompactLayout L) {
    const uint64_t c = blockIdx.x;
    const uint64_t ioff = 0;
    const uint8_t* in;
    int sn;
    CompactSlot stride, rec_stride;
    if (!compact_span(in_ptrs, in_bytes, c, max_bytes, L, in, sn, stride, rec_stride)) return;
    const uint32_t part = (uint32_t)sn;
    const uint64_t in_readable = (uint64_t)part + 16;
#include "pack_body.inc"
}

// ------------------------------------------------------------------------------------ launchers
hipError_t lzh_launch_compact_scans(const LzhCompactLayout& L, uint32_t nchunks, hipStream_t s) {
    const hipError_t e = lzh_launch_scan(L.stage_sz, nchunks, L.stage_off, nullptr, s);
    return e != hipSuccess ? e : lzh_launch_scan(L.rec_sz, nchunks, L.rec_off, nullptr, s);
}

hipError_t lzh_launch_compact_slots(int codec, const LzhBatch& B, const LzhCompactLayout& L, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_compact_slots_kernel, dim3((B.nchunks + 255) / 256), dim3(256), 0, s, B.bytes, B.max_bytes,
                       codec, L.stage_sz, L.rec_sz, B.nchunks);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : lzh_launch_compact_scans(L, B.nchunks, s);
}

hipError_t lzh_launch_lz4_compact(const LzhBatch& B, int acc, const LzhCompactSlots& S, uint32_t* csizes, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_lz4_parse_compact_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes, B.max_bytes, acc,
                       S.recs, S.hdr, S.L);
    hipLaunchKernelGGL(lzh_lz4_emit_compact_kernel, dim3(B.nchunks), dim3(64), 0, s, B.ptrs, B.bytes, B.max_bytes,
                       (const uint8_t*)S.recs, (const uint32_t*)S.hdr, S.stage, csizes, S.L);
    return hipGetLastError();
}

hipError_t lzh_launch_snappy_compact(const LzhBatch& B, const LzhCompactSlots& S, uint32_t* csizes, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    const uint32_t frags = lzh_snappy_ragged_frags(B.max_bytes);
    if (frags > (uint32_t)sne::kMaxFrags || (uint64_t)B.nchunks * frags > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lzh_snappy_parse_compact_kernel, dim3(B.nchunks * frags), dim3(64), 0, s, B.ptrs, B.bytes,
                       B.max_bytes, S.recs, S.hdr, frags, S.L);
    lzh_launch_snappy_emit(lzh_snappy_emit_compact_kernel, lzh_snappy_emit_frag_compact_kernel<2>,
                           lzh_snappy_emit_frag_compact_kernel<4>, lzh_snappy_emit_frag_compact_kernel<8>, frags, B.nchunks,
                           s, B.ptrs, B.bytes, B.max_bytes, S.recs, S.hdr, S.stage, csizes, frags, S.L);
    return hipGetLastError();
}

hipError_t lzh_launch_pack_compact(const LzhBatch& B, const LzhCompactSlots& S, const uint32_t* csizes,
                                   const uint64_t* offsets, uint8_t* packed, uint64_t packed_cap, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_pack_compact_kernel, dim3(B.nchunks), dim3(256), 0, s, B.ptrs, B.bytes, B.max_bytes,
                       (const uint8_t*)S.stage, csizes, offsets, packed, packed_cap, S.L);
    return hipGetLastError();
}
