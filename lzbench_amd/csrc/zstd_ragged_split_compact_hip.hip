// lzbench_amd/csrc/zstd_ragged_split_compact_hip.hip -- ragged zstd batches through the four-kernel split decoder in
// the compact temp layout (include/lzbench_hip.h 3g, lzh_zstd_decompress_ragged_split_compact_async): every frame's
// temp area is laid out for the frame's own decoded size and placed by an exclusive scan (zstd_split_slots.h), and
// the Huffman job list holds the sum of the frames' own block slots, so temp grows with the batch's total bytes.
// A unit of its own, built with the flags and the scheduler setting of zstd_ragged_split_hip.hip.  It includes that
// file as text for decode_hip.hip's device functions and the ragged geometry (RaggedPtrs, RaggedFrame), under
// LZH_ZSPLIT_GEOMETRY_ONLY, which leaves that unit's kernels and launchers out: no existing kernel shares a code object
// with the ones here (profiles and tests are keyed to their code hashes).
// In the terms of the csrc layout (tests/test_csrc_layout.py, profiles/decode_headers/README.md): the split decoder's
// device code stays in decode_hip.hip until zstd_ragged_split_hip.hip moves to headers, and that unit stays the one
// file that includes decode_hip.hip and names its include mode.  This unit is the second half of the same exception,
// not a second one: it reaches that device code only through the split unit, is the only file that includes it, and
// moves to the headers in the same step (tests/test_csrc_layout_split_compact.py holds it to that).
//
//   lzh_zstd_split_slots_kernel     frame i's area bytes and job slots (u32; 0 for a chunk over max_bytes)
//   lzh_launch_compact_scans        the two exclusive scans (ragged_compact_hip.hip: lzh_launch_scan twice)
//   lzh_zstd_split_states_kernel    the frame states: kGo; kDone and status -1 for a chunk over max_bytes; kLegacy
//                                   for a frame whose area or job slots end outside their regions (a batch that
//                                   breaks the promised total)
//   header, Huffman (4 / 8 sections a wave, long streams), sequences, execution: the bodies of the uniform-slot
//   kernels above, with a frame's area at areas + area_off[i] and its layout zlayout(the frame's own size)
//   lzh_launch_zstd_decompress_ragged_sel   the one-wave decoder over the frames left at kLegacy
//
// The layout struct is the compress side's LzhCompactLayout (launch.h) with other contents: stage_sz / stage_off /
// stage_cap carry the area sizes, their scan and the area region's bytes, rec_sz / rec_off / rec_cap the job counts,
// their scan and the job list's slots.
// A frame posts at most bmax(its own size) Huffman jobs -- the header kernel sends a frame of more blocks to
// kLegacy -- and the frames at kGo have disjoint runs of job slots inside the list, so the job counter never passes
// the list.

#define LZH_ZSPLIT_GEOMETRY_ONLY 1
#include "zstd_ragged_split_hip.hip"
#include "launch.h"
#include "zstd_split_slots.h"

namespace zsplit {
// zstdd_hdr_body.inc and zstdd_exec_body.inc name frame `chunk`'s area `zt + chunk * Z.stride`, with Z laid out for
// chunk_size.  Here chunk_size is the frame's own size and zt a Placed: the frame's own area, already placed by the
// scan, so whatever is added to it is dropped.  zstdd_seq_body.inc names the dummy words `zt + nchunks * Z.stride`
// in the same way: there zt is the dummy region, Placed.
struct Placed { uint8_t* base; };
__device__ __forceinline__ uint8_t* operator+(Placed a, uint64_t) { return a.base; }

// zstdd_hufpar_body.inc lays the temp out with zlayout(chunk_size), names the table slots of frame jf
// `zt + (uint64_t)jf * Z.stride + Z.hufs()` and its output `out + (uint64_t)jf * chunk_size`.  Here chunk_size is a
// CompactBytes, whose "layout" has a stride of 1 and no blocks -- jf * Z.stride is the frame's index and Z.hufs() is
// 0 -- and zt a HufTables: plus a frame's index, the frame's table slots (its area's scanned offset, then the
// blocks and sequence tables of the layout of its own size).  The output goes through RaggedPtrs, as above.
struct CompactBytes {};
__device__ __forceinline__ ZLayout zlayout(CompactBytes) { return ZLayout{0, 0, 1}; }
__device__ __forceinline__ RaggedFrame operator*(uint64_t frame, CompactBytes) { return RaggedFrame{frame}; }
struct HufTables {
    const uint8_t* areas;
    const uint64_t* area_off;
    const uint64_t* out_bytes;
};
__device__ __forceinline__ const uint8_t* operator+(HufTables t, uint64_t frame) {
    return t.areas + uni64(t.area_off[frame]) + zlayout(uni64(t.out_bytes[frame])).hufs();
}

// the compact geometry of zstd_huf: RaggedOut's output side; frame i's area at area_off[i] of zt (the area region),
// laid out for out_bytes[i]; the dummy words a region of their own
struct CompactOut {
    void* const* ptrs;
    const uint64_t* out_bytes;
    const uint64_t* area_off;
    uint8_t* dummies;
    uint32_t nchunks;
    __device__ __forceinline__ uint64_t frames() const { return nchunks; }
    __device__ __forceinline__ uint8_t* at(uint64_t frame) const { return (uint8_t*)ptrs[frame]; }
    __device__ __forceinline__ uint8_t* idle() const { return nullptr; }
    __device__ __forceinline__ ZLayout layout() const { return ZLayout{0, 0, 0}; }   // (none for the wave)
    __device__ __forceinline__ const uint8_t* area(const uint8_t* zt, uint32_t frame, const ZLayout&) const {
        return zt + uni64(area_off[frame]);
    }
    // (per lane; the scan is monotone, so the difference is the distance from the lowest frame's area.  A lane
    // without a job asks for frame 0, and the kernel ignores what it gets)
    __device__ __forceinline__ uint64_t tables(uint32_t frame, uint32_t fmin, const ZLayout&) const {
        return area_off[frame] - area_off[fmin] + zlayout(out_bytes[frame]).hufs();
    }
    __device__ __forceinline__ uint8_t* dummy(uint8_t*, uint64_t, const ZLayout&) const { return dummies; }
};

}  // namespace zsplit

// ------------------------------------------------------------------------------------------ placement
extern "C" __global__ void __launch_bounds__(256)
lzh_zstd_split_slots_kernel(const uint64_t* out_bytes, uint64_t max_bytes, uint32_t* area_sz, uint32_t* job_cnt,
                            uint32_t nchunks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchunks) return;
    const uint64_t b = out_bytes[i];
    const bool over = b > max_bytes;
    area_sz[i] = over ? 0u : (uint32_t)lzh_zsplit_area_bytes(b);
    job_cnt[i] = over ? 0u : (uint32_t)lzh_zsplit_jobs(b);
}

extern "C" __global__ void __launch_bounds__(256)
lzh_zstd_split_states_kernel(const uint64_t* out_bytes, uint64_t max_bytes, const LzhCompactLayout C, int32_t* zst,
                             int32_t* status, uint32_t nchunks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchunks) return;
    if (out_bytes[i] > max_bytes) {   // not processed: no other kernel looks at a frame that is kDone
        status[i] = -1;
        zst[i] = zsplit::kDone;
        return;
    }
    const bool in = C.stage_off[i] + C.stage_sz[i] <= C.stage_cap && C.rec_off[i] + C.rec_sz[i] <= C.rec_cap;
    zst[i] = in ? zsplit::kGo : zsplit::kLegacy;
}

// ------------------------------------------------------------------------------------------ the five kernels
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_hdr_compact_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                            const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                            int32_t* status, uint8_t* areas, const uint64_t* area_off, int32_t* zst, zsplit::ZFrame* zfr,
                            zsplit::ZHuf* jobs, uint32_t* njobs) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(zstdd::kLdsHdr + 3) / 4];
    LDSA zstdd::Lds& L = *(LDSA zstdd::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    if (uni((uint32_t)zst[chunk]) != (uint32_t)zsplit::kGo) return;   // (kDone: not processed; kLegacy: not placed)
    const uint8_t* outc;
    int sn;
    if (!ragged_span((const void* const*)out_ptrs, out_bytes, chunk, max_bytes, outc, sn)) return;
    uint8_t* out = (uint8_t*)outc;
    const uint64_t ooff = 0, n_total = (uint64_t)sn, chunk_size = (uint64_t)sn;
    const zsplit::Placed zt{areas + uni64(area_off[chunk])};
    unsigned long long* const stats = nullptr;
#include "zstdd_hdr_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_hufpar_compact_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                               void* const* out_ptrs, const uint64_t* out_bytes, int32_t* status, const uint8_t* areas,
                               const uint64_t* area_off, int32_t* zst, const zsplit::ZHuf* jobs, const uint32_t* njobs,
                               int par) {
    const zsplit::RaggedPtrs out{out_ptrs};
    const zsplit::CompactBytes chunk_size{};
    const zsplit::HufTables zt{areas, area_off, out_bytes};
#include "zstdd_hufpar_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_huf_compact_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                            void* const* out_ptrs, const uint64_t* out_bytes, uint32_t nchunks, int32_t* status,
                            uint8_t* areas, const uint64_t* area_off, uint8_t* dummies, int32_t* zst,
                            const zsplit::ZHuf* jobs, const uint32_t* njobs, int par) {
    zstd_huf<4>(packed, packed_readable, offsets, zsplit::CompactOut{out_ptrs, out_bytes, area_off, dummies, nchunks},
                status, areas, zst, jobs, njobs, nullptr, par);
}
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_huf8_compact_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                             void* const* out_ptrs, const uint64_t* out_bytes, uint32_t nchunks, int32_t* status,
                             uint8_t* areas, const uint64_t* area_off, uint8_t* dummies, int32_t* zst,
                             const zsplit::ZHuf* jobs, const uint32_t* njobs, int par) {
    zstd_huf<8>(packed, packed_readable, offsets, zsplit::CompactOut{out_ptrs, out_bytes, area_off, dummies, nchunks},
                status, areas, zst, jobs, njobs, nullptr, par);
}

// per lane: the layout of the lane's frame's own size and its area.  A lane without a frame parks at the area
// region's base with the layout of an empty frame and touches nothing there: its phase is "finished" from the
// start, it reads no block, and its stores go to its own word of the wave's dummy words.
extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_seq_compact_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                            const uint64_t* out_bytes, uint32_t nchunks, int32_t* status, uint8_t* areas,
                            const uint64_t* area_off, uint8_t* dummies, const int32_t* zst, zsplit::ZFrame* zfr) {
    using namespace zsplit;
    using namespace zstdd;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsSeq];
    LDSA uint8_t* const S = (LDSA uint8_t*)lds;
    const int lane = threadIdx.x;
    __builtin_amdgcn_s_setprio(3);   // (as lzh_zstd_seq_kernel)
    const int which = -1;            // (no plan: one launch over every frame)
    unsigned long long* const stats = nullptr;
    const uint32_t f0 = blockIdx.x * kFPW + (uint32_t)lane;
    const bool inl = lane < kFPW && f0 < nchunks;
    const uint32_t f = inl ? f0 : 0u;
    const bool live = inl && zst[f] == kGo;
    const ZLayout Z = zlayout(live ? out_bytes[f] : 0);
    uint8_t* const zb = areas + (live ? area_off[f] : 0);
    const Placed zt{dummies};
#include "zstdd_seq_body.inc"
}

extern "C" __global__ void __launch_bounds__(64)
lzh_zstd_exec_compact_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                             const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                             int32_t* status, uint8_t* areas, const uint64_t* area_off, int32_t* zst,
                             const zsplit::ZFrame* zfr) {
    __shared__ __attribute__((aligned(16))) uint8_t win[zstdd::kZW + 3 * LZH_WAVE];
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    if (zst[chunk] != zsplit::kGo) return;   // (the header / literal kernels' verdict first; kDone: not processed)
    const uint8_t* outc;
    int sn;
    if (!ragged_span((const void* const*)out_ptrs, out_bytes, chunk, max_bytes, outc, sn)) return;
    uint8_t* out = (uint8_t*)outc;
    const uint64_t ooff = 0, n_total = (uint64_t)sn, chunk_size = (uint64_t)sn;
    const zsplit::Placed zt{areas + uni64(area_off[chunk])};
#include "zstdd_exec_body.inc"
    if (lane == 0) zst[chunk] = zsplit::kDone;   // (as lzh_zstd_exec_ragged_kernel: kDone = finished here)
}

// ------------------------------------------------------------------------------------------ launcher
// Every launch on s, one chain: the placement (slot sizes, two scans, states), the job counter's memset, then the
// order of lzh_launch_zstd_decompress_ragged_split.  The Huffman grids are sized from the job list's slots
// (T.slots.rec_cap: total / 128 KiB + 2 x nchunks, or the uniform bound where smaller), which the host knows.
hipError_t lzh_launch_zstd_decompress_ragged_split_compact(const uint8_t* packed, uint64_t packed_readable,
                                                           const uint64_t* offsets, const uint32_t* csizes,
                                                           void* const* out_ptrs, const uint64_t* out_bytes,
                                                           uint64_t max_bytes, int32_t* status, uint32_t nchunks,
                                                           const LzhZstdSplitCompactTemp& T, hipStream_t s) {
    if (nchunks == 0) return hipSuccess;
    const LzhZstdHooks hooks = lzh_zstd_hooks(nchunks);
    if (hooks.legacy)
        return lzh_launch_zstd_decompress_ragged(packed, packed_readable, offsets, csizes, out_ptrs, out_bytes, max_bytes,
                                                 status, nchunks, s);
    const LzhCompactLayout& C = T.slots;
    int32_t* zst = T.state;
    zsplit::ZFrame* zfr = (zsplit::ZFrame*)T.zfr;
    zsplit::ZHuf* jobs = (zsplit::ZHuf*)T.jobs;
    const uint64_t maxjobs = C.rec_cap;
    const int hj = hooks.huf_sections;
    if (maxjobs == 0 || maxjobs * 4 > 0x7fffffffull) return hipErrorInvalidValue;   // (launch grids)
    const dim3 per_chunk((nchunks + 255) / 256);
    hipLaunchKernelGGL(lzh_zstd_split_slots_kernel, per_chunk, dim3(256), 0, s, out_bytes, max_bytes, C.stage_sz, C.rec_sz,
                       nchunks);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = lzh_launch_compact_scans(C, nchunks, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzh_zstd_split_states_kernel, per_chunk, dim3(256), 0, s, out_bytes, max_bytes, C, zst, status,
                       nchunks);
    e = hipMemsetAsync(T.njobs, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzh_zstd_hdr_compact_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets, csizes,
                       out_ptrs, out_bytes, max_bytes, status, T.areas, (const uint64_t*)C.stage_off, zst, zfr, jobs,
                       T.njobs);
    hipLaunchKernelGGL(hj == 8 ? lzh_zstd_huf8_compact_kernel : lzh_zstd_huf_compact_kernel,
                       dim3((unsigned)((maxjobs + hj - 1) / hj)), dim3(64), 0, s, packed, packed_readable, offsets,
                       out_ptrs, out_bytes, nchunks, status, T.areas, (const uint64_t*)C.stage_off, T.dummy, zst,
                       (const zsplit::ZHuf*)jobs, (const uint32_t*)T.njobs, hooks.hufpar);
    if (hooks.hufpar)   // (off: the per-lane kernel above decoded every stream)
        hipLaunchKernelGGL(lzh_zstd_hufpar_compact_kernel, dim3((unsigned)(maxjobs * 4)), dim3(64), 0, s, packed,
                           packed_readable, offsets, out_ptrs, out_bytes, status, (const uint8_t*)T.areas,
                           (const uint64_t*)C.stage_off, zst, (const zsplit::ZHuf*)jobs, (const uint32_t*)T.njobs,
                           hooks.hufpar);
    hipLaunchKernelGGL(lzh_zstd_seq_compact_kernel, dim3((nchunks + zsplit::kFPW - 1) / zsplit::kFPW), dim3(64), 0, s,
                       packed, packed_readable, offsets, out_bytes, nchunks, status, T.areas, (const uint64_t*)C.stage_off,
                       T.dummy, (const int32_t*)zst, zfr);
    hipLaunchKernelGGL(lzh_zstd_exec_compact_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets,
                       csizes, out_ptrs, out_bytes, max_bytes, status, T.areas, (const uint64_t*)C.stage_off, zst,
                       (const zsplit::ZFrame*)zfr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return lzh_launch_zstd_decompress_ragged_sel(packed, packed_readable, offsets, csizes, out_ptrs, out_bytes, max_bytes,
                                                 status, nchunks, (const int32_t*)zst, s);
}
