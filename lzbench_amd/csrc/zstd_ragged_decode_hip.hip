// lzbench_amd/csrc/zstd_ragged_decode_hip.hip -- zstd decoding of ragged batches (include/lzbench_hip.h 3c):
// frame i of the packed buffer decodes to the out_bytes[i] bytes at out_ptrs[i] (device arrays).
//
// The kernel is lzh_zstd_decompress_kernel of decode_hip.hip, the one-wave-per-frame decoder, with another chunk
// lookup: ragged_span (common.h) loads chunk blockIdx.x's output pointer and size once and makes them
// wave-uniform; what follows is that kernel's body (zstdd::decode_frame, a plain copy for a chunk stored raw).
// The frame is read and the output written through buffer descriptors of the frame's and the chunk's own sizes,
// so a malformed frame or a wrong size writes nothing outside the chunk.  The decoder's device code is zstdd.h,
// compiled here with decode_hip.hip's flags; nothing here changes the uniform decoders' code.
// A chunk whose device-side size passes max_bytes is not decoded: status -1, no byte written.
#include "decode_win.h"
#include "zstdd.h"

extern "C" __global__ void __launch_bounds__(64, LZH_ZSTD_MINW)
lzh_zstd_decompress_ragged_kernel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                  const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                                  uint64_t max_bytes, int32_t* status) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_raw[(sizeof(zstdd::Lds) + 3) / 4];
    LDSA zstdd::Lds& L = *(LDSA zstdd::Lds*)lds_raw;
    const int lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint8_t* outc;
    int part;
    if (!ragged_span((const void* const*)out_ptrs, out_bytes, chunk, max_bytes, outc, part)) {
        if (lane == 0) status[chunk] = -1;
        return;
    }
    uint8_t* out = (uint8_t*)outc;
    const uint64_t ioff = offsets[chunk];
    const int cs = (int)csizes[chunk];
    // (+16: whole-dword reads of the frame's last bytes; bytes past the frame are never used)
    const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, (uint64_t)cs + 16) : 0;
    Bytes rin, rout;
    rin.init(packed + ioff, readable);
    rout.init(out, (uint64_t)part);
    int r;
    if (cs == part) {                                  // stored raw (the raw-store rule of the compress calls)
        copy_raw(rin, rout, part, lane);
        r = part;
    } else {
        zstdd::ZSink O{(LDSA uint8_t*)L.win, rout, 0, 0};
        for (int i = lane; i < 36 + 53; i += LZH_WAVE) L.base[i] = i < 36 ? zstdd::kLLBase[i] : zstdd::kMLBase[i - 36];
        wave_lds_fence();
        Bytes lout;
        lout.init(out, (uint64_t)part + 3);
        r = zstdd::decode_frame(rin, lout, cs, O, L, part, lane, nullptr);
        if (r > 0) O.flush(r, lane);
    }
    if (lane == 0) status[chunk] = r;
}

#include "launch.h"

hipError_t lzh_launch_zstd_decompress_ragged(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                             const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                                             uint64_t max_bytes, int32_t* status, uint32_t nchunks, hipStream_t s) {
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(lzh_zstd_decompress_ragged_kernel, dim3(nchunks), dim3(64), 0, s, packed, packed_readable, offsets,
                       csizes, out_ptrs, out_bytes, max_bytes, status);
    return hipGetLastError();
}
