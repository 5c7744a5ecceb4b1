// lzbench_amd/csrc/lz4f_ragged_hip.hip -- ragged LZ4 frames on the device API (include/lzbench_hip.h 3i): one LZ4
// frame per chunk, the chunks given by device arrays of pointers and sizes.  Frame i is what LZ4F_compressFrame
// writes for chunk i alone with independent blocks, the bytes of the uniform call (frame_hip.hip) for a chunk size
// that holds the chunk.
//
// A ragged frame's block count is known only on the device, so the geometry is laid out for the largest chunk: with
// B the level's block size, bs = min(B, max_bytes) and bpf = ceil(max_bytes / bs), frame i owns the block slots
// i * bpf .. i * bpf + bpf - 1.  Compression:
//   lzh_lz4f_ragged_table_kernel   one lane per block slot: the derived block batch, slot i * bpf + j = (pointer of
//                                  chunk i + j * bs, min(bs, size - j * bs)); a slot past its frame's end, and every
//                                  slot of a chunk over max_bytes, gets a size above bs
//   (lzh_launch_lz4_ragged)        the ragged LZ4 parse and emit kernels of ragged_hip.hip over that batch with
//                                  max_bytes = bs: a slot with a size above bs is skipped, its block size is 0
//   lzh_lz4f_ragged_size_kernel    one lane per frame: frame size and block offsets, the raw-store rule on the frame
//   (lzh_launch_scan)              frame offsets
//   lzh_lz4f_ragged_pack_kernel    one workgroup per block slot (block word, stored bytes, block checksum) and one per
//                                  frame (header, end mark, content checksum; a raw-stored frame is copied here); a
//                                  frame whose packed range would pass packed_cap is not written
// Decompression: lzh_lz4f_ragged_parse_kernel (one wave per frame: header checks, block walk, block checksums) writes
// up to maxbpf = ceil(max_bytes / 64 KiB) descriptors per frame with absolute destination addresses for the block
// decoder (decode_hip.hip, descriptor mode with a null output base; linked frames through the same descriptors),
// lzh_lz4f_ragged_finish_kernel checks the blocks' results and the content checksum.  A chunk whose size passes
// max_bytes is not processed: csizes[i] = 0 / status[i] = -1, no kernel touches a slot or a byte for it.
// The frame format itself -- XXH32, header words, block walk -- is frame.h.
#include "frame.h"

// the size of chunk i, wave-uniform; false = it passes max_bytes
__device__ __forceinline__ bool frame_size_of(const uint64_t* bytes, uint64_t i, uint64_t max_bytes, uint64_t& s) {
    s = uni64(bytes[i]);
    return s <= max_bytes;
}

extern "C" __global__ void __launch_bounds__(256)
lzh_lz4f_ragged_table_kernel(const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes, uint64_t bs,
                             uint32_t bpf, uint64_t* tab_ptrs, uint64_t* tab_bytes, uint32_t nslots) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nslots) return;
    const uint32_t f = w / bpf, j = w - f * bpf;
    const uint64_t s = in_bytes[f], boff = (uint64_t)j * bs;
    const bool live = s <= max_bytes && boff < s;
    tab_ptrs[w] = live ? (uint64_t)in_ptrs[f] + boff : 0;
    tab_bytes[w] = live ? min(bs, s - boff) : bs + 1;
}

// one lane per frame: csizes[f] (0 for a chunk over max_bytes) and rel[] of its blocks
extern "C" __global__ void __launch_bounds__(256)
lzh_lz4f_ragged_size_kernel(int params, const uint64_t* in_bytes, uint64_t max_bytes, uint64_t bs, uint32_t bpf,
                            const uint32_t* bcs, uint32_t* rel, uint32_t* csizes, uint32_t nframes) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const uint64_t s = in_bytes[f];
    if (s > max_bytes) { csizes[f] = 0; return; }
    const uint32_t nb = (uint32_t)((s + bs - 1) / bs);
    const uint64_t pos = frm::lz4f_frame_bytes(params, s, bs, nb, bcs + (uint64_t)f * bpf, rel + (uint64_t)f * bpf);
    csizes[f] = pos == s ? (uint32_t)s : (uint32_t)pos;   // lzbench.cpp:284-288: clen == part -> raw
}

// grid (nblocks, 2): row 0 = one workgroup per block slot, row 1 = one per frame (the first nframes of the row)
extern "C" __global__ void __launch_bounds__(256)
lzh_lz4f_ragged_pack_kernel(int params, const void* const* in_ptrs, const uint64_t* in_bytes, uint64_t max_bytes,
                            uint64_t bs, uint32_t bpf, const uint8_t* stage, uint64_t stride, const uint32_t* bcs,
                            const uint32_t* rel, const uint32_t* csizes, const uint64_t* offsets, uint8_t* packed,
                            uint64_t packed_cap, uint32_t nframes) {
    const int t = threadIdx.x;
    const uint64_t w = blockIdx.x;
    const bool block_row = blockIdx.y == 0;
    const uint64_t f = block_row ? w / bpf : w;
    if (f >= nframes) return;
    uint64_t s;
    if (!frame_size_of(in_bytes, f, max_bytes, s)) return;
    const uint32_t fsz = uni(csizes[f]);
    const uint64_t foff = uni64(offsets[f]);
    if (foff + fsz > packed_cap) return;   // caller sized packed from offsets[nframes]
    const uint8_t* in = (const uint8_t*)uni64((uint64_t)in_ptrs[f]);
    if (block_row) {
        const uint64_t boff = (w - f * bpf) * bs;
        if (boff >= s || fsz == s) return;   // past the frame's end; frame stored raw
        const uint32_t bn = (uint32_t)min(bs, s - boff);
        const uint32_t c = bcs[w];
        const bool raw = c >= bn;
        const uint32_t st = raw ? bn : c;
        const int cb = (params >> 4) & 1 ? 4 : 0;
        Bytes src, dst;
        if (raw) src.init(in + boff, (uint64_t)bn + 16);
        else src.init(stage + w * stride, stride);
        dst.init(packed + foff + rel[w], (uint64_t)4 + st + cb);
        copy_span(src, 0, dst, 4, (int)st, t, blockDim.x);
        frm::lz4f_block_edges(src, dst, st, raw, cb, t);
        return;
    }
    Bytes src, dst;
    src.init(in, s + 16);
    dst.init(packed + foff, fsz);
    if (fsz == s) {   // raw-stored frame
        copy_span(src, 0, dst, 0, (int)s, t, blockDim.x);
        return;
    }
    if (t >= 64) return;
    frm::lz4f_frame_edges(params, src, s, bs, fsz, dst, t);
}

// ------------------------------------------------------------------------------------ decoding
// one wave per frame: maxbpf descriptor slots per frame (unused slots decode nothing), fstat[f] = 0 or a negative
// status; the frame decodes to out_bytes[f] bytes at out_ptrs[f]
extern "C" __global__ void __launch_bounds__(64)
lzh_lz4f_ragged_parse_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                             const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                             uint32_t maxbpf, FrameDesc* desc, int32_t* fstat) {
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    FrameDesc* D = desc + f * maxbpf;
    for (uint32_t b = (uint32_t)lane; b < maxbpf; b += 64) D[b] = FrameDesc{0, 0, 0, 0, 0, 0};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the zeroing before lane 0's descriptor stores
    __syncthreads();
    uint64_t s;
    if (!frame_size_of(out_bytes, f, max_bytes, s)) {
        if (lane == 0) fstat[f] = -1;
        return;
    }
    const uint64_t ioff = uni64(offsets[f]);
    const uint64_t dst = uni64((uint64_t)out_ptrs[f]);
    const uint32_t cs = uni(csizes[f]);
    if (cs == s) {   // stored raw by the chunk loop (lzbench.cpp:318-321)
        if (lane == 0) { D[0] = FrameDesc{ioff, dst, cs, (uint32_t)s, 1, 0}; fstat[f] = 0; }
        return;
    }
    Bytes fr;
    const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, (uint64_t)cs + 16) : 0;
    fr.init(packed + ioff, readable);
    const int st = frm::lz4f_parse(fr, packed + ioff, readable, ioff, cs, s, dst, D, lane);
    if (lane == 0) fstat[f] = st;
}

// one wave per frame: the blocks' decoded sizes, the content checksum -> status[f]
extern "C" __global__ void __launch_bounds__(64)
lzh_lz4f_ragged_finish_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                              const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                              uint64_t max_bytes, uint32_t maxbpf, const FrameDesc* desc, const int32_t* bstat,
                              const int32_t* fstat, int32_t* status) {
    const int lane = threadIdx.x;
    const uint64_t f = blockIdx.x;
    uint64_t s;
    if (!frame_size_of(out_bytes, f, max_bytes, s)) {
        if (lane == 0) status[f] = -1;
        return;
    }
    int st = frm::blocks_verdict(fstat[f], desc + f * maxbpf, bstat + f * maxbpf, maxbpf, lane);
    const uint32_t cs = uni(csizes[f]);
    if (!st && cs != s) {
        const uint64_t ioff = uni64(offsets[f]);
        const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, cs) : 0;
        const uint8_t* out = (const uint8_t*)uni64((uint64_t)out_ptrs[f]);
        if (!frm::lz4f_content_ok(packed + ioff, cs, readable, out, s, lane)) st = -1;
    }
    if (lane == 0) status[f] = st ? st : (int32_t)s;
}

#include "launch.h"

hipError_t lzh_launch_lz4f_ragged(const LzhBatch& B, int acc, const LzhRaggedFrame& R, uint32_t* csizes, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    const uint32_t nslots = B.nchunks * R.bpf;
    hipLaunchKernelGGL(lzh_lz4f_ragged_table_kernel, dim3((nslots + 255) / 256), dim3(256), 0, s, B.ptrs, B.bytes,
                       B.max_bytes, R.bs, R.bpf, (uint64_t*)R.bptrs, R.bbytes, nslots);
    const LzhBatch blocks = {R.bptrs, R.bbytes, R.bs, nslots};
    const hipError_t e = lzh_launch_lz4_ragged(blocks, acc, R.F.blocks, R.F.bcs, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzh_lz4f_ragged_size_kernel, dim3((B.nchunks + 255) / 256), dim3(256), 0, s, R.params, B.bytes,
                       B.max_bytes, R.bs, R.bpf, (const uint32_t*)R.F.bcs, R.F.rel, csizes, B.nchunks);
    return hipGetLastError();
}

hipError_t lzh_launch_lz4f_pack_ragged(const LzhBatch& B, const LzhRaggedFrame& R, const uint32_t* csizes,
                                       const uint64_t* offsets, uint8_t* packed, uint64_t packed_cap, hipStream_t s) {
    if (B.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_lz4f_ragged_pack_kernel, dim3(B.nchunks * R.bpf, 2), dim3(256), 0, s, R.params, B.ptrs, B.bytes,
                       B.max_bytes, R.bs, R.bpf, (const uint8_t*)R.F.blocks.stage, R.F.blocks.stride,
                       (const uint32_t*)R.F.bcs, (const uint32_t*)R.F.rel, csizes, offsets, packed, packed_cap, B.nchunks);
    return hipGetLastError();
}

hipError_t lzh_launch_lz4f_decompress_ragged(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                             const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                                             uint64_t max_bytes, int32_t* status, uint32_t nchunks, uint32_t maxbpf,
                                             void* desc, int32_t* bstat, int32_t* fstat, hipStream_t s) {
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_lz4f_ragged_parse_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets, csizes,
                       out_ptrs, out_bytes, max_bytes, maxbpf, (FrameDesc*)desc, fstat);
    // (the block decoder adds the descriptor's destination, the block's address, to a null output base)
    const hipError_t e = lzh_launch_decompress(0, packed, packed_readable, nullptr, nullptr, 0, 0, nullptr, bstat,
                                               nchunks * maxbpf, s, desc);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzh_lz4f_ragged_finish_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets, csizes,
                       out_ptrs, out_bytes, max_bytes, maxbpf, (const FrameDesc*)desc, (const int32_t*)bstat,
                       (const int32_t*)fstat, status);
    return hipGetLastError();
}
