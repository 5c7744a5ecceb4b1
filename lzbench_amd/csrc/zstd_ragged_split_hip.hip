// lzbench_amd/csrc/zstd_ragged_split_hip.hip -- ragged zstd batches (include/lzbench_hip.h 3c) through the
// four-kernel split decoder of decode_hip.hip: header, Huffman literals (a stream per lane, long streams a wave
// each), sequences, execution; then the one-wave-per-frame decoder over the frames those leave at kLegacy.
//
// The kernels are the uniform ones with another frame lookup.  Their bodies are decode_hip.hip's, shared as text
// (zstdd_hdr_body.inc, zstdd_hufpar_body.inc, zstdd_exec_body.inc, zstdd_frame_body.inc) or as a template over the
// output geometry (zstd_huf): the only things that differ are where a frame's output is -- out_ptrs[i] /
// out_bytes[i], loaded once and made wave-uniform by ragged_span (common.h) -- and what the per-frame temp slots
// are sized for (max_bytes).  The sequence kernel never sees the output, so the uniform lzh_zstd_seq_kernel runs as
// it is (lzh_launch_zstd_seq).  The frame is read and the output written through buffer descriptors of the frame's
// and the chunk's own sizes, so a malformed frame or a wrong size writes nothing outside the chunk; the Huffman
// kernels write through raw pointers, inside the literal area the header kernel checked against the chunk's own
// size.  decode_hip.hip is included for its device functions alone (and compiled with its flags), in a unit of its
// own: nothing here changes the code of the uniform decoders or of lzh_zstd_decompress_ragged_kernel
// (profiles/traffic*.json are keyed to their code hashes).
// A chunk whose device-side size passes max_bytes is not decoded: status -1, frame state kDone, no byte of its
// frame read, of its output or of its temp slot written.
#define LZH_DEVICE_FUNCTIONS_ONLY 2   // (the split decoder's device functions as well)
#include "decode_hip.hip"

namespace zsplit {
// the ragged geometry of zstd_huf: frame i's output at ptrs[i]; every temp slot sized for max_bytes; nchunks frames
struct RaggedOut {
    void* const* ptrs;
    uint64_t max_bytes;
    uint32_t nchunks;
    __device__ __forceinline__ uint64_t slot() const { return max_bytes; }
    __device__ __forceinline__ uint64_t frames() const { return nchunks; }
    __device__ __forceinline__ uint8_t* at(uint64_t frame) const { return (uint8_t*)ptrs[frame]; }
    __device__ __forceinline__ uint8_t* idle() const { return nullptr; }
    // (the temp side: uniform slots, as UniformOut's)
    __device__ __forceinline__ ZLayout layout() const { return zlayout(slot()); }
    __device__ __forceinline__ const uint8_t* area(const uint8_t* zt, uint32_t frame, const ZLayout& Z) const {
        return zt + (uint64_t)frame * Z.stride;
    }
    __device__ __forceinline__ uint64_t tables(uint32_t frame, uint32_t fmin, const ZLayout& Z) const {
        return (uint64_t)(frame - fmin) * Z.stride + Z.hufs();
    }
    __device__ __forceinline__ uint8_t* dummy(uint8_t* zt, uint64_t nfr, const ZLayout& Z) const { return zt + nfr * Z.stride; }
};
// zstdd_hufpar_body.inc names the output of frame jf `out + (uint64_t)jf * chunk_size` and lays the temp out with
// zlayout(chunk_size).  Here `out` is the batch's pointer array and `chunk_size` a RaggedSlotBytes: an integer times
// it is that frame's index, the pointer array plus a frame's index the frame's pointer, and its conversion to an
// integer max_bytes (nothing else compiles).
struct RaggedSlotBytes {
    uint64_t max_bytes;
    __device__ __forceinline__ operator uint64_t() const { return max_bytes; }
};
struct RaggedFrame { uint64_t index; };
struct RaggedPtrs { void* const* ptrs; };
__device__ __forceinline__ RaggedFrame operator*(uint64_t frame, RaggedSlotBytes) { return RaggedFrame{frame}; }
__device__ __forceinline__ uint8_t* operator+(RaggedPtrs p, RaggedFrame f) { return (uint8_t*)p.ptrs[f.index]; }
}  // namespace zsplit

// (zstd_ragged_split_compact_hip.hip includes this file up to here, for decode_hip.hip's device functions and the
// geometry above: the kernels and launchers below are this unit's alone)
#ifndef LZH_ZSPLIT_GEOMETRY_ONLY
// The header and execution kernels run the uniform kernels' bodies under the names those use: chunk's output is
// out + ooff with ooff = 0, its size min(chunk_size, n_total - ooff) with n_total the chunk's own size and
// chunk_size = max_bytes, for which the per-frame temp is laid out.
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_hdr_ragged_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                           const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                           int32_t* status, uint8_t* zt, int32_t* zst, zsplit::ZFrame* zfr, zsplit::ZHuf* jobs,
                           uint32_t* njobs) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(zstdd::kLdsHdr + 3) / 4];
    LDSA zstdd::Lds& L = *(LDSA zstdd::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint8_t* outc;
    int sn;
    if (!ragged_span((const void* const*)out_ptrs, out_bytes, chunk, max_bytes, outc, sn)) {
        if (lane == 0) {   // not processed: no other kernel looks at a frame that is kDone
            status[chunk] = -1;
            zst[chunk] = zsplit::kDone;
        }
        return;
    }
    uint8_t* out = (uint8_t*)outc;
    const uint64_t ooff = 0, n_total = (uint64_t)sn, chunk_size = max_bytes;
    unsigned long long* const stats = nullptr;
#include "zstdd_hdr_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_hufpar_ragged_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                              void* const* out_ptrs, uint64_t max_bytes, int32_t* status, uint8_t* zt, int32_t* zst,
                              const zsplit::ZHuf* jobs, const uint32_t* njobs, int par) {
    const zsplit::RaggedPtrs out{out_ptrs};
    const zsplit::RaggedSlotBytes chunk_size{max_bytes};
#include "zstdd_hufpar_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_huf_ragged_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                           void* const* out_ptrs, uint64_t max_bytes, uint32_t nchunks, int32_t* status, uint8_t* zt,
                           int32_t* zst, const zsplit::ZHuf* jobs, const uint32_t* njobs, int par) {
    zstd_huf<4>(packed, packed_readable, offsets, zsplit::RaggedOut{out_ptrs, max_bytes, nchunks}, status, zt, zst, jobs,
                njobs, nullptr, par);
}
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_huf8_ragged_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                            void* const* out_ptrs, uint64_t max_bytes, uint32_t nchunks, int32_t* status, uint8_t* zt,
                            int32_t* zst, const zsplit::ZHuf* jobs, const uint32_t* njobs, int par) {
    zstd_huf<8>(packed, packed_readable, offsets, zsplit::RaggedOut{out_ptrs, max_bytes, nchunks}, status, zt, zst, jobs,
                njobs, nullptr, par);
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_exec_ragged_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                            const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                            int32_t* status, const uint8_t* zt, int32_t* zst, const zsplit::ZFrame* zfr) {
    __shared__ __attribute__((aligned(16))) uint8_t win[zstdd::kZW + 3 * LZH_WAVE];
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    if (zst[chunk] != zsplit::kGo) return;   // (the header / literal kernels' verdict first; kDone: not processed)
    const uint8_t* outc;
    int sn;
    if (!ragged_span((const void* const*)out_ptrs, out_bytes, chunk, max_bytes, outc, sn)) return;
    uint8_t* out = (uint8_t*)outc;
    const uint64_t ooff = 0, n_total = (uint64_t)sn, chunk_size = max_bytes;
#include "zstdd_exec_body.inc"
    // (executed, whatever the verdict: the states then read kDone = finished here, kLegacy = the one-wave kernel's;
    // the uniform kernel leaves such a frame at kGo, which nothing reads afterwards)
    if (lane == 0) zst[chunk] = zsplit::kDone;
}

#ifndef LZH_ZSTD_MINW
#define LZH_ZSTD_MINW 1   // waves per SIMD the register allocation must allow (as lzh_zstd_decompress_kernel)
#endif
// the one-wave decoder (lzh_zstd_decompress_ragged_kernel of zstd_ragged_decode_hip.hip) over the frames the split
// kernels left at kLegacy (zsel: their frame states; kDone: decoded, refused or not processed)
extern "C" __global__ void __launch_bounds__(64, LZH_ZSTD_MINW)
lzh_zstd_decompress_ragged_sel_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                      const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                                      uint64_t max_bytes, int32_t* status, const int32_t* zsel) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(sizeof(zstdd::Lds) + 3) / 4];
    LDSA zstdd::Lds& L = *(LDSA zstdd::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    if (zsel[chunk] != zsplit::kLegacy) return;
    const uint8_t* outc;
    int part;
    if (!ragged_span((const void* const*)out_ptrs, out_bytes, chunk, max_bytes, outc, part)) return;
    uint8_t* out = (uint8_t*)outc;
    const uint64_t ooff = 0;
    unsigned long long* const stats = nullptr;
#include "zstdd_frame_body.inc"
}

#include "launch.h"
#include "zstd_split_slots.h"

// the area arithmetic of the compact temp layout (zstd_split_slots.h) for api.cpp, which cannot include
// decode_hip.hip, where the layout it derives from (zsplit::zlayout) lives: the two regions, and the area and job
// slots of a frame of n bytes.  Host arithmetic; zstd_ragged_split_compact_hip.hip decodes through that layout.
LzhZsplitRegions lzh_zstd_split_compact_regions(uint64_t total, uint64_t max_bytes, uint64_t nchunks) {
    return lzh_zsplit_regions(total, max_bytes, nchunks);
}
LzhZsplitRegions lzh_zstd_split_compact_slot(uint64_t n) { return {lzh_zsplit_area_bytes(n), lzh_zsplit_jobs(n)}; }

// Every launch on s, in the order of the uniform launcher with everything on one stream: the job counter's memset,
// header, Huffman streams a lane each (4 or 8 sections a wave), long streams a wave each, sequences, execution, then
// the one-wave kernel over the frames left at kLegacy.  No side stream, event, plan kernel or host synchronisation:
// a captured call is one chain.
hipError_t lzh_launch_zstd_decompress_ragged_split(const uint8_t* packed, uint64_t packed_readable,
                                                   const uint64_t* offsets, const uint32_t* csizes,
                                                   void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                                                   int32_t* status, uint32_t nchunks, const LzhZstdSplitTemp& split,
                                                   hipStream_t s) {
    if (nchunks == 0) return hipSuccess;
    const LzhZstdHooks hooks = lzh_zstd_hooks(nchunks);
    if (hooks.legacy)
        return lzh_launch_zstd_decompress_ragged(packed, packed_readable, offsets, csizes, out_ptrs, out_bytes, max_bytes,
                                                 status, nchunks, s);
    uint8_t* zt = split.frames;
    int32_t* zst = split.state;
    zsplit::ZFrame* zfr = (zsplit::ZFrame*)split.zfr;
    zsplit::ZHuf* jobs = (zsplit::ZHuf*)split.jobs;
    uint32_t* njobs = split.njobs;
    const uint64_t maxjobs = (uint64_t)nchunks * zsplit::zlayout(max_bytes).bmax;
    const int hj = hooks.huf_sections;
    if (maxjobs * 4 > 0x7fffffffull) return hipErrorInvalidValue;   // (launch grids)
    hipError_t e = hipMemsetAsync(njobs, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzh_zstd_hdr_ragged_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets, csizes,
                       out_ptrs, out_bytes, max_bytes, status, zt, zst, zfr, jobs, njobs);
    hipLaunchKernelGGL(hj == 8 ? lzh_zstd_huf8_ragged_kernel : lzh_zstd_huf_ragged_kernel,
                       dim3((unsigned)((maxjobs + hj - 1) / hj)), dim3(64), 0, s, packed, packed_readable, offsets,
                       out_ptrs, max_bytes, nchunks, status, zt, zst, (const zsplit::ZHuf*)jobs, (const uint32_t*)njobs,
                       hooks.hufpar);
    if (hooks.hufpar)   // (off: the per-lane kernel above decoded every stream)
        hipLaunchKernelGGL(lzh_zstd_hufpar_ragged_kernel, dim3((unsigned)(maxjobs * 4)), dim3(64), 0, s, packed,
                           packed_readable, offsets, out_ptrs, max_bytes, status, zt, zst, (const zsplit::ZHuf*)jobs,
                           (const uint32_t*)njobs, hooks.hufpar);
    e = lzh_launch_zstd_seq(packed, packed_readable, offsets, max_bytes, nchunks, status, zt, zst, zfr, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzh_zstd_exec_ragged_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets,
                       csizes, out_ptrs, out_bytes, max_bytes, status, (const uint8_t*)zt, zst, (const zsplit::ZFrame*)zfr);
    hipLaunchKernelGGL(lzh_zstd_decompress_ragged_sel_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable,
                       offsets, csizes, out_ptrs, out_bytes, max_bytes, status, (const int32_t*)zst);
    return hipGetLastError();
}

// the one-wave kernel over the frames at kLegacy alone (zsel: the frame states), for the compact layout's launcher
hipError_t lzh_launch_zstd_decompress_ragged_sel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                                 const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                                                 uint64_t max_bytes, int32_t* status, uint32_t nchunks,
                                                 const int32_t* zsel, hipStream_t s) {
    hipLaunchKernelGGL(lzh_zstd_decompress_ragged_sel_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable,
                       offsets, csizes, out_ptrs, out_bytes, max_bytes, status, zsel);
    return hipGetLastError();
}
#endif   // LZH_ZSPLIT_GEOMETRY_ONLY
