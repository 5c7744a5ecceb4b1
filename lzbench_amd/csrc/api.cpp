// lzbench_amd/csrc/api.cpp -- the C-ABI of include/lzbench_hip.h.
//
// Device-resident layer: stage -> scan -> pack for compression, scan -> decode for
// decompression, all asynchronous on the caller's stream.
// Host layer: lzbench rows and batched rows.  A row's workmem is an LzhCtx holding, per GPU,
// a stream and device buffers sized at init for the chunk size (grown on demand).  A batch
// is cut into runs of uniform chunking (lzbench's chunk list is uniform per input file,
// lzbench.cpp:366-373); each run is cut into ~128 MiB sub-batches dealt round-robin to the GPUs
// (make_plan), every GPU pipelines its sub-batches (copy in | kernels | copy out), and the host
// places each sub-batch's packed bytes at its chunk-order offset as soon as the sizes before it
// are known.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include <rocprofiler-sdk-roctx/roctx.h>

#include "../../include/lzbench_hip.h"
#include "launch.h"
#include "ragged_slots.h"
#include "temp_layout.h"

static_assert(kLzhSlotLz4 == LZH_CODEC_LZ4 && kLzhSlotSnappy == LZH_CODEC_SNAPPY, "ragged_slots.h: codec numbers");

// rocprof-visible ranges around each stage's launches (rocprofv3 --marker-trace); a range covers
// the enqueue of the stage on the host, the kernels themselves show in --kernel-trace
struct Range {
    explicit Range(const char* n) { roctxRangePushA(n); }
    ~Range() { roctxRangePop(); }
};

extern "C" size_t lzb_datagen(int kind, uint64_t seed, uint8_t* buf, size_t n);

#define LZH_CHECK(x)                                                                  \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "lzbench_hip: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return LZH_EHIP;                                                          \
        }                                                                             \
    } while (0)

extern "C" {

const char* lzh_version(void) { return "lzbench_hip 0.2 (lz4 1.9.3 / snappy 1.1.8 / zstd 1.5.2 fast levels + level 3 bit-exact, gfx950)"; }

size_t lzh_datagen(int kind, uint64_t seed, void* buf, size_t n) { return lzb_datagen(kind, seed, (uint8_t*)buf, n); }

size_t lzh_num_chunks(size_t n, size_t chunk_size) {
    if (chunk_size == 0) return 0;
    return n == 0 ? 1 : (n + chunk_size - 1) / chunk_size;
}

static bool is_frame(int codec) { return codec == LZH_CODEC_LZ4F || codec == LZH_CODEC_NVLZ4; }

static size_t codec_bound(int codec, size_t part) {
    if (codec == LZH_CODEC_LZ4F)    // raw blocks at worst, 64 KiB blocks the smallest: header, block words, end
        return part + 8 * ((part + 65535) / 65536) + 32;
    if (codec == LZH_CODEC_NVLZ4)   // LZ4 blocks of 32 KiB at the least, 8-byte fields
        return part + part / 255 + 24 * ((part + 32767) / 32768) + 48;
    if (codec == LZH_CODEC_LZ4) return part + part / 255 + 16;     // LZ4_compressBound, lz4.h:171
    if (codec == LZH_CODEC_SNAPPY) return 32 + part + part / 6;    // MaxCompressedLength, snappy.cc:99-121
    if (codec == LZH_CODEC_ZSTD || codec == LZH_CODEC_ZSTD_DFAST)   // ZSTD_COMPRESSBOUND, zstd.h:~210
        return part + (part >> 8) + (part < (128u << 10) ? ((128u << 10) - part) >> 11 : 0);
    return part;
}

size_t lzh_stage_stride(int codec, size_t chunk_size) { return align_up(codec_bound(codec, chunk_size) + 16, 256); }

size_t lzh_max_packed_bytes(int codec, size_t n, size_t chunk_size) {
    size_t k = lzh_num_chunks(n, chunk_size);
    return n + k * (codec_bound(codec, chunk_size) - chunk_size + 8) + 64;
}

// Framed layouts: frames of F bytes (the chunks) cut into blocks of bs = min(F, B) bytes (FrameGeo, temp_layout.h)
static size_t frame_block_bytes(int codec, int level) {
    if (codec == LZH_CODEC_LZ4F) { const int id = level & 7; return (size_t)1 << (8 + 2 * (id ? id : 4)); }
    return (size_t)32768 << level;
}

static bool frame_level_ok(int codec, int level) {
    if (codec == LZH_CODEC_LZ4F) { const int id = level & 7; return level >= 0 && level < (1 << 16) && (id == 0 || id >= 4) && !(level & 0x08); }
    return level >= 0 && level <= 5;
}

extern "C" int lzh_level_supported(int codec, int level, size_t chunk_size) {
    if (codec == LZH_CODEC_ZSTD) return lzh_zstd_level_ok(level, chunk_size) ? 1 : 0;
    if (codec == LZH_CODEC_ZSTD_DFAST) return level == 3 ? 1 : 0;   // (dfast in all four clevels tables)
    if (codec == LZH_CODEC_LZ4F || codec == LZH_CODEC_NVLZ4) return frame_level_ok(codec, level) ? 1 : 0;
    return codec >= LZH_CODEC_LZ4 && codec <= LZH_CODEC_MEMCPY ? 1 : 0;
}

// (the sizing call does not know the level: the largest temp of the block sizes a level can select)
static size_t frame_temp_worst(int codec, size_t n, size_t F) {
    size_t t = 0;
    for (int l = 0; l < 6; l++) {
        const size_t B = codec == LZH_CODEC_LZ4F ? ((size_t)65536 << (2 * std::min(l, 3))) : ((size_t)32768 << l);
        t = std::max(t, frame_temp(frame_geo(B, n, F)).total);
    }
    return t;
}

size_t lzh_compress_temp_bytes(int codec, size_t n, size_t chunk_size) {
    if (codec == LZH_CODEC_MEMCPY) return 256;
    if (is_frame(codec)) return frame_temp_worst(codec, n, chunk_size) + 256;
    return chunk_temp(codec, lzh_num_chunks(n, chunk_size), chunk_size).total;
}

// (LZH_CODEC_ZSTD_DFAST writes LZH_CODEC_ZSTD's frames: one decoder)
static int decode_codec(int codec) { return codec == LZH_CODEC_ZSTD_DFAST ? LZH_CODEC_ZSTD : codec; }

size_t lzh_decompress_temp_bytes(int codec, size_t n, size_t chunk_size) {
    return decode_temp(decode_codec(codec), n, chunk_size).total;
}

// ---- the uniform compress calls: one input buffer cut at chunk_size ----
// chunk counts and sizes the kernels hold in 32 bits
static bool fits_u32(size_t k, size_t chunk_size) { return k <= 0xffffffffu && chunk_size <= 0x7fff0000u; }

// the codec takes the level, and n bytes in chunks of chunk_size
static bool uniform_ok(int codec, int level, size_t n, size_t chunk_size) {
    if (!fits_u32(lzh_num_chunks(n, chunk_size), chunk_size)) return false;
    if (codec == LZH_CODEC_LZ4 || codec == LZH_CODEC_SNAPPY) return true;
    if (is_frame(codec)) return frame_level_ok(codec, level);
    if (codec == LZH_CODEC_ZSTD) return lzh_zstd_level_ok(level, chunk_size) != 0;
    return codec == LZH_CODEC_ZSTD_DFAST && level == 3 && chunk_size <= kLz4SplitMax;
}

// What a uniform compress call hands its launchers, formed once, after the argument checks (uniform_ok): the input
// and the slots of the call's layout in temp -- chunk_temp, where F.blocks alone is set; for a framed codec frame_temp
// of the level's geometry, where I's chunks are the blocks.
struct UniformCall {
    LzhInput I;
    LzhFrameSlots F;
    bool split;   // LZ4 / snappy: parse -> records -> emit
};
static UniformCall uniform_call(int codec, int level, const void* d_in, size_t n, size_t in_readable, size_t chunk_size,
                                const void* temp) {
    const uint8_t* in = (const uint8_t*)d_in;
    uint8_t* base = (uint8_t*)temp;   // (const in lzh_compress_finish_async, which only reads the staging slots)
    if (is_frame(codec)) {
        const FrameGeo g = frame_geo(frame_block_bytes(codec, level), n, chunk_size);
        return {{in, n, in_readable, g.bs, (uint32_t)g.nblocks, g.F, g.bpf, (uint32_t)g.nframes}, frame_temp(g).slots(base),
                true};
    }
    const size_t k = lzh_num_chunks(n, chunk_size);
    const ChunkTemp t = chunk_temp(codec, k, chunk_size);
    return {{in, n, in_readable, chunk_size, (uint32_t)k, 0, 1, (uint32_t)k}, {t.slots(base), nullptr, nullptr},
            t.split};
}

// the compress kernels of the call; stage_mask bit 0: parse / the whole compression, bit 1: emit, frame sizes
static int uniform_kernels(int codec, int level, int stage_mask, const UniformCall& c, uint32_t* d_csizes, hipStream_t s) {
    const LzhInput& I = c.I;
    const LzhSlots& S = c.F.blocks;
    Range range("lzh:compress_kernel");
    if (codec == LZH_CODEC_LZ4) {
        const int acc = level < 1 ? 1 : level;
        if (c.split) LZH_CHECK(lzh_launch_lz4_split(I, acc, S, d_csizes, stage_mask, s));
        else if (stage_mask & 1) LZH_CHECK(lzh_launch_lz4_compress_v2(I, acc, S, d_csizes, s));
    } else if (codec == LZH_CODEC_SNAPPY) {
        if (c.split) LZH_CHECK(lzh_launch_snappy_split(I, S, d_csizes, stage_mask, s));
        else if (stage_mask & 1) LZH_CHECK(lzh_launch_snappy_compress_v2(I, S, d_csizes, s));
    } else if (is_frame(codec)) {   // blocks -> frame sizes (d_csizes)
        const int acc = codec == LZH_CODEC_LZ4F ? std::max(1, (level >> 8) & 0xff) : 1;
        if (codec == LZH_CODEC_LZ4F && (level & LZH_LZ4F_LINKED)) {
            // linked blocks: one wave per frame walks its blocks in order (the records area holds the
            // per-frame table snapshots: 16 KiB per frame)
            if (stage_mask & 1) LZH_CHECK(lzh_launch_lz4f_linked(I, acc, c.F, s));
        } else {
            LZH_CHECK(lzh_launch_lz4_split(I, acc, S, c.F.bcs, stage_mask, s));
        }
        if (stage_mask & 2) LZH_CHECK(lzh_launch_frame_sizes(I, codec, level, c.F.bcs, c.F.rel, d_csizes, s));
    } else if (codec == LZH_CODEC_ZSTD) {
        if (stage_mask & 1) LZH_CHECK(lzh_launch_zstd_compress(I, level, S, d_csizes, s));
    } else {   // LZH_CODEC_ZSTD_DFAST: match + entropy per block index, every launch on s
        LZH_CHECK(lzh_launch_zstd_dfast_compress(I, level, S, d_csizes, s));
    }
    return LZH_OK;
}

// sizes -> offsets -> the chunks (frames) back to back in d_packed
static int uniform_scan_pack(int codec, int level, const UniformCall& c, const uint32_t* d_csizes, uint64_t* d_offsets,
                             void* d_packed, size_t packed_cap, hipStream_t s) {
    Range range("lzh:scan_pack");
    LZH_CHECK(lzh_launch_scan(d_csizes, c.I.nframes, d_offsets, nullptr, s));
    if (is_frame(codec)) {
        LZH_CHECK(lzh_launch_frame_pack(c.I, codec, level, c.F, d_csizes, d_offsets, (uint8_t*)d_packed, s));
    } else if (codec == LZH_CODEC_ZSTD_DFAST && c.I.n_total == 0) {
        // (the pack kernel looks chunks up in the input and finds none in an empty one: the one frame of an empty
        // input -- magic, descriptor, a content size of 0, an empty last raw block -- is copied as it is)
        const size_t kEmptyFrame = 4 + 1 + 1 + 3;
        LZH_CHECK(lzh_launch_memcpy(c.F.blocks.stage, d_packed, kEmptyFrame, s));
    } else {
        LZH_CHECK(lzh_launch_pack(c.I, c.F.blocks, d_csizes, d_offsets, (uint8_t*)d_packed, packed_cap, s));
    }
    return LZH_OK;
}

// (d_stage = the whole compression temp; framed layouts: d_csizes = frame sizes)
int lzh_compress_kernel_stage(int codec, int level, int stage_mask, const void* d_in, size_t n, size_t in_readable,
                              size_t chunk_size, void* d_stage, uint32_t* d_csizes, void* hip_stream) {
    if (!chunk_size || !d_stage || !d_csizes || (n && !d_in)) return LZH_EARG;
    if (codec == LZH_CODEC_ZSTD_DFAST || !uniform_ok(codec, level, n, chunk_size)) return LZH_EARG;
    return uniform_kernels(codec, level, stage_mask, uniform_call(codec, level, d_in, n, in_readable, chunk_size, d_stage),
                           d_csizes, (hipStream_t)hip_stream);
}

int lzh_compress_kernel_only(int codec, int level, const void* d_in, size_t n, size_t in_readable,
                             size_t chunk_size, void* d_stage, uint32_t* d_csizes, void* hip_stream) {
    if (is_frame(codec)) return LZH_EARG;   // (framed layouts: lzh_compress_async)
    return lzh_compress_kernel_stage(codec, level, 3, d_in, n, in_readable, chunk_size, d_stage, d_csizes, hip_stream);
}

__global__ void lzh_fill_raw_sizes(uint32_t* cs, uint64_t k, uint64_t n, uint64_t chunk) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) cs[i] = (uint32_t)std::min<uint64_t>(chunk, n - i * chunk);
}

int lzh_compress_async(int codec, int level, const void* d_in, size_t n, size_t in_readable, size_t chunk_size,
                       void* d_packed, size_t packed_cap, uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp,
                       size_t temp_bytes, void* hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    if (!chunk_size || !d_packed || !d_csizes || !d_offsets || (n && !d_in)) return LZH_EARG;
    if (in_readable < n) return LZH_EARG;
    if (codec == LZH_CODEC_MEMCPY) {
        const size_t k = lzh_num_chunks(n, chunk_size);
        if (packed_cap < n) return LZH_ESPACE;
        if (n == 0) return LZH_OK;
        hipLaunchKernelGGL(lzh_fill_raw_sizes, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, s, d_csizes,
                           (uint64_t)k, (uint64_t)n, (uint64_t)chunk_size);
        LZH_CHECK(hipGetLastError());
        LZH_CHECK(lzh_launch_scan(d_csizes, k, d_offsets, nullptr, s));
        LZH_CHECK(lzh_launch_memcpy(d_in, d_packed, n, s));
        return LZH_OK;
    }
    if (temp_bytes < lzh_compress_temp_bytes(codec, n, chunk_size) || !d_temp) return LZH_ESPACE;
    if (packed_cap < lzh_max_packed_bytes(codec, n, chunk_size)) return LZH_ESPACE;
    if (!uniform_ok(codec, level, n, chunk_size)) return LZH_EARG;
    const UniformCall c = uniform_call(codec, level, d_in, n, in_readable, chunk_size, d_temp);
    const int rc = uniform_kernels(codec, level, 3, c, d_csizes, s);
    return rc ? rc : uniform_scan_pack(codec, level, c, d_csizes, d_offsets, d_packed, packed_cap, s);
}

int lzh_compress_finish_async(int codec, const void* d_in, size_t n, size_t in_readable, size_t chunk_size,
                              const void* d_stage, const uint32_t* d_csizes, void* d_packed, size_t packed_cap,
                              uint64_t* d_offsets, void* hip_stream) {
    if (!chunk_size || !d_stage || !d_csizes || !d_packed || !d_offsets) return LZH_EARG;
    if (codec != LZH_CODEC_LZ4 && codec != LZH_CODEC_SNAPPY && codec != LZH_CODEC_ZSTD) return LZH_EARG;
    // the sizes are only known on the device: the worst case must fit (no silent truncation)
    if (packed_cap < lzh_max_packed_bytes(codec, n, chunk_size)) return LZH_ESPACE;
    return uniform_scan_pack(codec, 0, uniform_call(codec, 0, d_in, n, in_readable, chunk_size, d_stage), d_csizes,
                             d_offsets, d_packed, packed_cap, (hipStream_t)hip_stream);
}

int lzh_decompress_async(int codec, const void* d_packed, size_t packed_readable, const uint32_t* d_csizes,
                         const uint64_t* d_offsets, size_t n, size_t chunk_size, void* d_out, int32_t* d_status,
                         void* d_temp, size_t temp_bytes, void* hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    if (!chunk_size || !d_csizes || !d_status || (n && (!d_out || !d_packed))) return LZH_EARG;
    codec = decode_codec(codec);
    if (codec < 0 || codec > LZH_CODEC_NVLZ4) return LZH_EARG;
    if (codec == LZH_CODEC_ZSTD && chunk_size > (1u << 30)) return LZH_EARG;
    const size_t k = lzh_num_chunks(n, chunk_size);
    if (n == 0) return LZH_OK;
    Range range("lzh:decompress");
    const uint64_t* offs = d_offsets;
    const DecodeTemp t = decode_temp(codec, n, chunk_size);
    uint8_t* base = (uint8_t*)d_temp;
    if (is_frame(codec) && (!d_temp || temp_bytes < t.total)) return LZH_ESPACE;
    if (!offs && (!d_temp || temp_bytes < t.need_scan)) return LZH_ESPACE;
    // zstd, snappy chunks of several 64 KiB fragments: the split decoder's layout lives in temp after the offsets;
    // without room for it (or for chunks it does not take) every chunk is decoded whole by one wave
    uint8_t* split = d_temp && t.need_split && temp_bytes >= t.need_split ? base + t.split : nullptr;
    if (!offs) {
        LZH_CHECK(lzh_launch_scan(d_csizes, k, (uint64_t*)(base + t.scan), nullptr, s));
        offs = (const uint64_t*)(base + t.scan);
    }
    if (is_frame(codec)) {   // frame headers -> block descriptors -> blocks -> frame checks
        if (!fits_u32(k, chunk_size)) return LZH_EARG;
        const uint32_t mb = frame_maxbpf(codec, chunk_size);
        const size_t nd = k * mb;
        void* desc = base + t.desc;
        int32_t* bstat = (int32_t*)(base + t.bstat);
        int32_t* fstat = (int32_t*)(base + t.fstat);
        if (nd > 0xffffffffu) return LZH_EARG;
        LZH_CHECK(lzh_launch_frame_parse(codec, (const uint8_t*)d_packed, packed_readable, offs, d_csizes, n, chunk_size,
                                         mb, desc, fstat, (uint32_t)k, s));
        LZH_CHECK(lzh_launch_decompress(LZH_CODEC_LZ4, (const uint8_t*)d_packed, packed_readable, nullptr, nullptr, n,
                                        chunk_size, (uint8_t*)d_out, bstat, (uint32_t)nd, s, desc));
        LZH_CHECK(lzh_launch_frame_finish(codec, (const uint8_t*)d_packed, offs, d_csizes, n, chunk_size, mb, desc,
                                          bstat, fstat, (const uint8_t*)d_out, d_status, (uint32_t)k, s));
        return LZH_OK;
    }
    if (codec == LZH_CODEC_ZSTD)
        LZH_CHECK(lzh_launch_zstd_decompress((const uint8_t*)d_packed, packed_readable, offs, d_csizes, n, chunk_size,
                                             (uint8_t*)d_out, d_status, (uint32_t)k, split, s));
    else if (split)   // (snappy: a fragment per wave)
        LZH_CHECK(lzh_launch_snappy_split_decompress((const uint8_t*)d_packed, packed_readable, offs, d_csizes, n,
                                                     chunk_size, (uint8_t*)d_out, d_status, (uint32_t)k, split, s));
    else
        LZH_CHECK(lzh_launch_decompress(codec, (const uint8_t*)d_packed, packed_readable, offs, d_csizes, n,
                                        chunk_size, (uint8_t*)d_out, d_status, (uint32_t)k, s));
    return LZH_OK;
}

// ---- 3b. ragged batches: chunk i = d_in_bytes[i] bytes at d_in_ptrs[i] (device arrays) ----
// compress temp: chunk_temp of nchunks slots sized for max_chunk_bytes; decompress temp: ragged_decode_temp

static bool ragged_ok(int codec, size_t max_chunk_bytes) {
    return (codec == LZH_CODEC_LZ4 || codec == LZH_CODEC_SNAPPY) && max_chunk_bytes <= kLz4SplitMax;
}

size_t lzh_ragged_compress_temp_bytes(int codec, size_t max_chunk_bytes, size_t nchunks) {
    return ragged_ok(codec, max_chunk_bytes) ? chunk_temp(codec, nchunks, max_chunk_bytes).total : 0;
}

size_t lzh_ragged_decompress_temp_bytes(int codec, size_t max_chunk_bytes, size_t nchunks) {
    return ragged_ok(codec, max_chunk_bytes) ? ragged_decode_temp(nchunks).total : 0;
}

size_t lzh_ragged_max_packed_bytes(int codec, size_t total_in_bytes, size_t nchunks) {
    // the sum of codec_bound over the chunks, whatever their sizes: the bounds are linear in the size but for
    // their constant; then the uniform call's 8 bytes per chunk and 64
    const size_t var = codec == LZH_CODEC_LZ4 ? total_in_bytes / 255 : codec == LZH_CODEC_SNAPPY ? total_in_bytes / 6 : 0;
    return total_in_bytes + var + nchunks * (codec_bound(codec, 0) + 8) + 64;
}

}  // extern "C"

// the pack launcher of a layout's slots
static hipError_t launch_pack(const LzhBatch& B, const LzhSlots& S, const uint32_t* csizes, const uint64_t* offsets,
                              uint8_t* packed, uint64_t packed_cap, hipStream_t s) {
    return lzh_launch_pack_ragged(B, S, csizes, offsets, packed, packed_cap, s);
}
static hipError_t launch_pack(const LzhBatch& B, const LzhCompactSlots& S, const uint32_t* csizes, const uint64_t* offsets,
                              uint8_t* packed, uint64_t packed_cap, hipStream_t s) {
    return lzh_launch_pack_compact(B, S, csizes, offsets, packed, packed_cap, s);
}
static hipError_t launch_pack(const LzhBatch& B, const LzhRaggedFrame& R, const uint32_t* csizes, const uint64_t* offsets,
                              uint8_t* packed, uint64_t packed_cap, hipStream_t s) {
    return lzh_launch_lz4f_pack_ragged(B, R, csizes, offsets, packed, packed_cap, s);
}

// The ragged compress calls (3b .. 3h; uniform slots, compact layout): the argument checks in their order (ok: the
// codec / level takes max_chunk_bytes; have_dict: the dictionary's pointer, true for a call without one; grid_factor:
// launch blocks per chunk; t: the call's layout, its total the temp needed), then launch(B, S, s) -> scan -> the pack
// of the layout's slots, all enqueued on the stream.  B is the batch and S the layout's slots in d_temp, formed only
// after d_temp has been checked: the launch runs after that too, and adds what offsets of t it needs itself.
template <class Temp, class Launch>
static int ragged_compress(bool ok, bool have_dict, size_t grid_factor, const Temp& t, const void* const* d_in_ptrs,
                           const uint64_t* d_in_bytes, size_t nchunks, size_t max_chunk_bytes, void* d_packed,
                           size_t packed_cap, uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp, size_t temp_bytes,
                           void* hip_stream, Launch launch) {
    if (!ok) return LZH_EARG;
    if (nchunks == 0) return LZH_OK;
    if (!(have_dict && d_in_ptrs && d_in_bytes && d_packed && d_csizes && d_offsets && d_temp)) return LZH_EARG;
    if (nchunks * grid_factor > 0x7fffffffu) return LZH_EARG;   // launch grids
    if (temp_bytes < t.total) return LZH_ESPACE;
    hipStream_t s = (hipStream_t)hip_stream;
    const LzhBatch B = {d_in_ptrs, d_in_bytes, max_chunk_bytes, (uint32_t)nchunks};
    const auto S = t.slots((uint8_t*)d_temp);
    {
        Range range("lzh:compress_kernel");
        LZH_CHECK(launch(B, S, s));
    }
    Range range("lzh:scan_pack");
    LZH_CHECK(lzh_launch_scan(d_csizes, nchunks, d_offsets, nullptr, s));
    LZH_CHECK(launch_pack(B, S, d_csizes, d_offsets, (uint8_t*)d_packed, packed_cap, s));
    return LZH_OK;
}

// The ragged decompress calls: the argument checks in their order (grid_factor: launch blocks per chunk; t: the call's
// layout, its total the temp needed, the scanned offsets at t.scan), then decode(offs, t) with the caller's offsets or,
// without them, the ones scanned into temp.
template <class Decode>
static int ragged_decompress(bool ok, size_t nchunks, size_t grid_factor, const DecodeTemp& t, bool pointers,
                             const uint32_t* d_csizes, const uint64_t* d_offsets, void* d_temp, size_t temp_bytes,
                             hipStream_t s, Decode decode) {
    if (!ok) return LZH_EARG;
    if (nchunks == 0) return LZH_OK;
    if (!pointers) return LZH_EARG;
    if (nchunks * grid_factor > 0x7fffffffu) return LZH_EARG;   // launch grids
    if (temp_bytes < t.total) return LZH_ESPACE;
    Range range("lzh:decompress");
    const uint64_t* offs = d_offsets;
    if (!offs) {
        LZH_CHECK(lzh_launch_scan(d_csizes, nchunks, (uint64_t*)((uint8_t*)d_temp + t.scan), nullptr, s));
        offs = (const uint64_t*)((uint8_t*)d_temp + t.scan);
    }
    LZH_CHECK(decode(offs, t));
    return LZH_OK;
}

// The debug calls of the two compact layouts: the two regions (zstd: recs = scratch), and the host mirror of the
// slot placement (the slot-size kernel, the two scans, compact_span; slot(n): a chunk's two slot sizes)
static int compact_regions_out(bool ok, const CompactTemp& t, uint64_t* out) {
    if (!ok || !out) return LZH_EARG;
    out[0] = t.stage;
    out[1] = t.reg.stage;
    out[2] = t.recs;
    out[3] = t.reg.recs;
    return LZH_OK;
}

template <class Slot>
static int compact_slots_mirror(bool ok, const LzhCompactRegions& reg, const uint64_t* sizes, size_t nchunks,
                                size_t max_chunk_bytes, uint64_t* stage_off, uint64_t* rec_off, uint8_t* processed,
                                Slot slot) {
    if (!ok) return LZH_EARG;
    if (nchunks == 0) return LZH_OK;
    if (!sizes || !stage_off || !rec_off || !processed) return LZH_EARG;
    uint64_t so = 0, ro = 0;
    for (size_t i = 0; i < nchunks; i++) {
        const bool over = sizes[i] > max_chunk_bytes;
        const LzhCompactRegions sz = over ? LzhCompactRegions{0, 0} : slot(sizes[i]);
        stage_off[i] = so;
        rec_off[i] = ro;
        processed[i] = !over && so + sz.stage <= reg.stage && ro + sz.recs <= reg.recs;
        so += sz.stage;
        ro += sz.recs;
    }
    return LZH_OK;
}

extern "C" {

int lzh_compress_ragged_async(int codec, int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                              size_t nchunks, size_t max_chunk_bytes, void* d_packed, size_t packed_cap,
                              uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp, size_t temp_bytes,
                              void* hip_stream) {
    return ragged_compress(ragged_ok(codec, max_chunk_bytes), true, lzh_snappy_ragged_frags(max_chunk_bytes),
                           chunk_temp(codec, nchunks, max_chunk_bytes), d_in_ptrs, d_in_bytes, nchunks, max_chunk_bytes,
                           d_packed, packed_cap, d_csizes, d_offsets, d_temp, temp_bytes, hip_stream,
                           [&](const LzhBatch& B, const LzhSlots& S, hipStream_t s) {
                               return codec == LZH_CODEC_LZ4 ? lzh_launch_lz4_ragged(B, level < 1 ? 1 : level, S, d_csizes, s)
                                                             : lzh_launch_snappy_ragged(B, S, d_csizes, s);
                           });
}

int lzh_decompress_ragged_async(int codec, const void* d_packed, size_t packed_readable, const uint32_t* d_csizes,
                                const uint64_t* d_offsets, void* const* d_out_ptrs, const uint64_t* d_out_bytes,
                                size_t nchunks, size_t max_chunk_bytes, int32_t* d_status, void* d_temp,
                                size_t temp_bytes, void* hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    return ragged_decompress(
        ragged_ok(codec, max_chunk_bytes), nchunks, 1, ragged_decode_temp(nchunks),
        d_packed && d_csizes && d_out_ptrs && d_out_bytes && d_status && d_temp, d_csizes, d_offsets, d_temp, temp_bytes, s,
        [&](const uint64_t* offs, const DecodeTemp& t) {
            void* desc = (uint8_t*)d_temp + t.desc;
            const hipError_t e = lzh_launch_ragged_desc(offs, d_csizes, d_out_ptrs, d_out_bytes, max_chunk_bytes, desc,
                                                        d_status, (uint32_t)nchunks, s);
            if (e != hipSuccess) return e;
            // (the block decoder adds the descriptor's destination, the chunk's address, to a null output base)
            return lzh_launch_decompress(codec, (const uint8_t*)d_packed, packed_readable, nullptr, nullptr, 0, 0, nullptr,
                                         d_status, (uint32_t)nchunks, s, desc);
        });
}

// ---- 3d. LZ4 ragged batches with a shared dictionary: lz4_dict_temp / ragged_decode_temp, the checks and the
// scan -> pack of 3b ----
static bool lz4_dict_ok(size_t dict_bytes, size_t max_chunk_bytes) {
    return dict_bytes >= 8 && dict_bytes <= 65536 && max_chunk_bytes <= kLz4DictMax;
}

size_t lzh_lz4_dict_compress_temp_bytes(size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks) {
    return lz4_dict_ok(dict_bytes, max_chunk_bytes) ? lz4_dict_temp(nchunks, max_chunk_bytes).total : 0;
}

size_t lzh_lz4_dict_decompress_temp_bytes(size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks) {
    return lz4_dict_ok(dict_bytes, max_chunk_bytes) ? ragged_decode_temp(nchunks).total : 0;
}

int lzh_lz4_compress_ragged_dict_async(int level, const void* d_dict, size_t dict_bytes,
                                       const void* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t nchunks,
                                       size_t max_chunk_bytes, void* d_packed, size_t packed_cap, uint32_t* d_csizes,
                                       uint64_t* d_offsets, void* d_temp, size_t temp_bytes, void* hip_stream) {
    const DictTemp t = lz4_dict_temp(nchunks, max_chunk_bytes);
    const int acc = level < 1 ? 1 : std::min(level, 65537);   // (LZ4_ACCELERATION_MAX, lz4.c:1578)
    return ragged_compress(lz4_dict_ok(dict_bytes, max_chunk_bytes), d_dict != nullptr, 1, t, d_in_ptrs, d_in_bytes, nchunks,
                           max_chunk_bytes, d_packed, packed_cap, d_csizes, d_offsets, d_temp, temp_bytes, hip_stream,
                           [&](const LzhBatch& B, const LzhSlots& S, hipStream_t s) {
                               return lzh_launch_lz4_dict((const uint8_t*)d_dict, (uint32_t)dict_bytes,
                                                          (uint32_t*)((uint8_t*)d_temp + t.tab), B, acc, S, d_csizes, s);
                           });
}

int lzh_lz4_decompress_ragged_dict_async(const void* d_dict, size_t dict_bytes, const void* d_packed,
                                         size_t packed_readable, const uint32_t* d_csizes, const uint64_t* d_offsets,
                                         void* const* d_out_ptrs, const uint64_t* d_out_bytes, size_t nchunks,
                                         size_t max_chunk_bytes, int32_t* d_status, void* d_temp, size_t temp_bytes,
                                         void* hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    return ragged_decompress(
        lz4_dict_ok(dict_bytes, max_chunk_bytes), nchunks, 1, ragged_decode_temp(nchunks),
        d_dict && d_packed && d_csizes && d_out_ptrs && d_out_bytes && d_status && d_temp, d_csizes, d_offsets, d_temp,
        temp_bytes, s, [&](const uint64_t* offs, const DecodeTemp&) {
            return lzh_launch_lz4_dict_decompress((const uint8_t*)d_dict, (uint32_t)dict_bytes, (const uint8_t*)d_packed,
                                                  packed_readable, offs, d_csizes, d_out_ptrs, d_out_bytes,
                                                  max_chunk_bytes, d_status, (uint32_t)nchunks, s);
        });
}

// ---- 3f. ragged zstd batches with a shared dictionary: zstd_dict_temp / ragged_decode_temp, the checks and the
// scan -> pack of 3c ----
static bool zstd_dict_sizes_ok(size_t dict_bytes, size_t max_chunk_bytes) {
    return dict_bytes >= 8 && dict_bytes <= kZstdDictMax && max_chunk_bytes <= kZstdDictMax;
}
static bool zstd_dict_ok(int level, size_t dict_bytes, size_t max_chunk_bytes) {
    return (level == 1 || (level <= -1 && level >= -5)) && zstd_dict_sizes_ok(dict_bytes, max_chunk_bytes);
}

size_t lzh_zstd_dict_compress_temp_bytes(int level, size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks) {
    return zstd_dict_ok(level, dict_bytes, max_chunk_bytes) ? zstd_dict_temp(dict_bytes, nchunks, max_chunk_bytes).total : 0;
}

size_t lzh_zstd_dict_decompress_temp_bytes(size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks) {
    return zstd_dict_sizes_ok(dict_bytes, max_chunk_bytes) ? ragged_decode_temp(nchunks).total : 0;
}

// the pointer checks of the two host-walk debug calls
static bool dict_parse_pointers(const void* dict, const void* src, size_t n, const uint32_t* seqs, size_t cap) {
    return dict && (src || !n) && (seqs || !cap);
}

int lzh_zstd_compress_ragged_dict_async(int level, const void* d_dict, size_t dict_bytes, const void* const* d_in_ptrs,
                                        const uint64_t* d_in_bytes, size_t nchunks, size_t max_chunk_bytes,
                                        void* d_packed, size_t packed_cap, uint32_t* d_csizes, uint64_t* d_offsets,
                                        void* d_temp, size_t temp_bytes, void* hip_stream) {
    const bool ok = zstd_dict_ok(level, dict_bytes, max_chunk_bytes);
    const ZstdDictTemp t = ok ? zstd_dict_temp(dict_bytes, nchunks, max_chunk_bytes) : ZstdDictTemp{};
    return ragged_compress(ok, d_dict != nullptr, 1, t, d_in_ptrs, d_in_bytes, nchunks, max_chunk_bytes, d_packed,
                           packed_cap, d_csizes, d_offsets, d_temp, temp_bytes, hip_stream,
                           [&](const LzhBatch& B, const LzhSlots& S, hipStream_t s) {
                               return lzh_launch_zstd_dict((const uint8_t*)d_dict, (uint32_t)dict_bytes,
                                                           (uint8_t*)d_temp + t.tabs, B, level, S, d_csizes, s);
                           });
}

int lzh_zstd_decompress_ragged_dict_async(const void* d_dict, size_t dict_bytes, const void* d_packed,
                                          size_t packed_readable, const uint32_t* d_csizes, const uint64_t* d_offsets,
                                          void* const* d_out_ptrs, const uint64_t* d_out_bytes, size_t nchunks,
                                          size_t max_chunk_bytes, int32_t* d_status, void* d_temp, size_t temp_bytes,
                                          void* hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    return ragged_decompress(
        zstd_dict_sizes_ok(dict_bytes, max_chunk_bytes), nchunks, 1, ragged_decode_temp(nchunks),
        d_dict && d_packed && d_csizes && d_out_ptrs && d_out_bytes && d_status && d_temp, d_csizes, d_offsets, d_temp,
        temp_bytes, s, [&](const uint64_t* offs, const DecodeTemp&) {
            return lzh_launch_zstd_dict_decompress((const uint8_t*)d_dict, (uint32_t)dict_bytes, (const uint8_t*)d_packed,
                                                   packed_readable, offs, d_csizes, d_out_ptrs, d_out_bytes,
                                                   max_chunk_bytes, d_status, (uint32_t)nchunks, s);
        });
}

int lzh_debug_zstd_dict_params(int level, size_t n, size_t dict_bytes, uint32_t* out) {
    if (!out || !zstd_dict_ok(level, dict_bytes, n)) return LZH_EARG;
    return lzh_zstd_dict_params(level, n, dict_bytes, out) ? LZH_OK : LZH_EARG;
}

long lzh_debug_zstd_dict_parse(int level, const void* dict, size_t dict_bytes, const void* src, size_t n, uint32_t* seqs,
                               size_t cap) {
    if (!dict_parse_pointers(dict, src, n, seqs, cap) || !zstd_dict_ok(level, dict_bytes, n)) return LZH_EARG;
    return lzh_zstd_dict_host_parse(level, (const uint8_t*)dict, dict_bytes, (const uint8_t*)src, n, seqs, cap);
}

// ---- 3h. ragged zstd level-3 batches with a shared dictionary: zstd_dfast_dict_temp, 3f's checks with level 3 alone,
// the scan -> pack of 3c; the frames decode with 3f's call ----
static bool zstd_dfast_dict_ok(int level, size_t dict_bytes, size_t max_chunk_bytes) {
    return level == 3 && zstd_dict_sizes_ok(dict_bytes, max_chunk_bytes);
}

size_t lzh_zstd_dfast_dict_compress_temp_bytes(int level, size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks) {
    return zstd_dfast_dict_ok(level, dict_bytes, max_chunk_bytes)
               ? zstd_dfast_dict_temp(dict_bytes, nchunks, max_chunk_bytes).total : 0;
}

int lzh_zstd_dfast_compress_ragged_dict_async(int level, const void* d_dict, size_t dict_bytes,
                                              const void* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t nchunks,
                                              size_t max_chunk_bytes, void* d_packed, size_t packed_cap,
                                              uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp, size_t temp_bytes,
                                              void* hip_stream) {
    const bool ok = zstd_dfast_dict_ok(level, dict_bytes, max_chunk_bytes);
    const ZstdDictTemp t = ok ? zstd_dfast_dict_temp(dict_bytes, nchunks, max_chunk_bytes) : ZstdDictTemp{};
    return ragged_compress(ok, d_dict != nullptr, 1, t, d_in_ptrs, d_in_bytes, nchunks, max_chunk_bytes, d_packed,
                           packed_cap, d_csizes, d_offsets, d_temp, temp_bytes, hip_stream,
                           [&](const LzhBatch& B, const LzhSlots& S, hipStream_t s) {
                               return lzh_launch_zstd_dfast_dict((const uint8_t*)d_dict, (uint32_t)dict_bytes,
                                                                 (uint8_t*)d_temp + t.tabs, B, level, S, d_csizes, s);
                           });
}

int lzh_debug_zstd_dfast_dict_params(int level, size_t n, size_t dict_bytes, uint32_t* out) {
    if (!out || !zstd_dfast_dict_ok(level, dict_bytes, n)) return LZH_EARG;
    return lzh_zstd_dfast_dict_params(level, n, dict_bytes, out) ? LZH_OK : LZH_EARG;
}

long lzh_debug_zstd_dfast_dict_parse(int level, const void* dict, size_t dict_bytes, const void* src, size_t n,
                                     uint32_t* seqs, size_t cap, uint64_t* events) {
    if (!dict_parse_pointers(dict, src, n, seqs, cap) || !zstd_dfast_dict_ok(level, dict_bytes, n)) return LZH_EARG;
    return lzh_zstd_dfast_dict_host_parse(level, (const uint8_t*)dict, dict_bytes, (const uint8_t*)src, n, seqs, cap,
                                          events);
}

// ---- 3c. ragged zstd batches: entry points of their own (the calls of 3b keep refusing zstd) ----
// compress temp: chunk_temp(zstd) of nchunks staging slots and scratch areas sized for max_chunk_bytes;
// decompress temp: ragged_decode_temp (its scanned offsets; the one-wave decoder needs no descriptors), or
// zstd_ragged_split_temp, with which the four-kernel split decoder runs

static bool zstd_ragged_ok(int level, size_t max_chunk_bytes) {
    return max_chunk_bytes <= kLz4SplitMax && lzh_level_supported(LZH_CODEC_ZSTD, level, max_chunk_bytes) == 1;
}

// (a batch of empty chunks is laid out as one of 1-byte chunks, here and in lzh_launch_zstd_ragged: size 0 is
// ZSTD_getParams' "unknown size", whose parameters would size every slot for a full 128 KiB block)
static ChunkTemp zstd_ragged_temp(size_t nchunks, size_t max_chunk_bytes) {
    return chunk_temp(LZH_CODEC_ZSTD, nchunks, std::max<size_t>(max_chunk_bytes, 1));
}

size_t lzh_zstd_ragged_compress_temp_bytes(int level, size_t max_chunk_bytes, size_t nchunks) {
    return zstd_ragged_ok(level, max_chunk_bytes) ? zstd_ragged_temp(nchunks, max_chunk_bytes).total : 0;
}

size_t lzh_zstd_ragged_decompress_temp_bytes(size_t max_chunk_bytes, size_t nchunks) {
    return max_chunk_bytes <= kLz4SplitMax ? ragged_decode_temp(nchunks).total : 0;
}

size_t lzh_zstd_ragged_decompress_split_temp_bytes(size_t max_chunk_bytes, size_t nchunks) {
    return zstd_ragged_split_temp(nchunks, max_chunk_bytes).total;
}

int lzh_debug_zstd_ragged_split_layout(size_t max_chunk_bytes, size_t nchunks, uint64_t* out) {
    const ZstdRaggedSplitTemp t = zstd_ragged_split_temp(nchunks, max_chunk_bytes);
    if (!t.ok || !out) return LZH_EARG;
    const uint64_t v[14] = {t.scan,   (nchunks + 1) * sizeof(uint64_t), t.frames, t.frames_bytes, t.dummy, t.dummy_bytes,
                            t.state,  t.state_bytes,                    t.fields, t.fields_bytes, t.njobs, 4,
                            t.jobs,   t.jobs_bytes};
    std::copy(v, v + 14, out);
    out[14] = t.stride;
    out[15] = t.total;
    return LZH_OK;
}

size_t lzh_zstd_ragged_max_packed_bytes(size_t total_in_bytes, size_t nchunks) {
    // the sum of codec_bound (the bound lzh_stage_stride sizes a slot for) over the chunks, whatever their sizes:
    // size + size / 256 + at most codec_bound(0) = 64 (a chunk of 1..64 bytes becomes size + 9 and is not stored
    // raw); then the uniform call's 8 bytes per chunk and 64
    return total_in_bytes + (total_in_bytes >> 8) + nchunks * (codec_bound(LZH_CODEC_ZSTD, 0) + 8) + 64;
}

int lzh_zstd_compress_ragged_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t nchunks,
                                   size_t max_chunk_bytes, void* d_packed, size_t packed_cap, uint32_t* d_csizes,
                                   uint64_t* d_offsets, void* d_temp, size_t temp_bytes, void* hip_stream) {
    return ragged_compress(zstd_ragged_ok(level, max_chunk_bytes), true, 1, zstd_ragged_temp(nchunks, max_chunk_bytes),
                           d_in_ptrs, d_in_bytes, nchunks, max_chunk_bytes, d_packed, packed_cap, d_csizes, d_offsets, d_temp,
                           temp_bytes, hip_stream, [&](const LzhBatch& B, const LzhSlots& S, hipStream_t s) {
                               return lzh_launch_zstd_ragged(B, level, S, d_csizes, s);
                           });
}

int lzh_zstd_decompress_ragged_async(const void* d_packed, size_t packed_readable, const uint32_t* d_csizes,
                                     const uint64_t* d_offsets, void* const* d_out_ptrs, const uint64_t* d_out_bytes,
                                     size_t nchunks, size_t max_chunk_bytes, int32_t* d_status, void* d_temp,
                                     size_t temp_bytes, void* hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    return ragged_decompress(
        max_chunk_bytes <= kLz4SplitMax, nchunks, 1, ragged_decode_temp(nchunks),
        d_packed && d_csizes && d_out_ptrs && d_out_bytes && d_status && d_temp, d_csizes, d_offsets, d_temp, temp_bytes, s,
        [&](const uint64_t* offs, const DecodeTemp&) {
            // with room for it the split decoder's layout lives in temp (the offsets at the same place); with less
            // every frame is decoded whole by one wave
            const ZstdRaggedSplitTemp z = zstd_ragged_split_temp(nchunks, max_chunk_bytes);
            uint8_t* base = (uint8_t*)d_temp;
            if (z.ok && temp_bytes >= z.total) {
                const LzhZstdSplitTemp split = {base + z.frames, (int32_t*)(base + z.state), base + z.fields,
                                                (uint32_t*)(base + z.njobs), base + z.jobs};
                return lzh_launch_zstd_decompress_ragged_split((const uint8_t*)d_packed, packed_readable, offs, d_csizes,
                                                               d_out_ptrs, d_out_bytes, max_chunk_bytes, d_status,
                                                               (uint32_t)nchunks, split, s);
            }
            return lzh_launch_zstd_decompress_ragged((const uint8_t*)d_packed, packed_readable, offs, d_csizes, d_out_ptrs,
                                                     d_out_bytes, max_chunk_bytes, d_status, (uint32_t)nchunks, s);
        });
}

// ---- 3c, compact layout of the split decoder's temp, the debug calls (3g below decodes through it): every frame's
// area laid out for its own size and placed by a scan (zstd_split_slots.h); zstd_ragged_split_compact_temp lays the
// temp out ----
int lzh_debug_zstd_ragged_split_compact_layout(size_t total_out_bytes, size_t max_chunk_bytes, size_t nchunks,
                                               uint64_t* out) {
    const ZstdRaggedSplitCompactTemp t = zstd_ragged_split_compact_temp(total_out_bytes, max_chunk_bytes, nchunks);
    if (!t.ok || !out) return LZH_EARG;
    const uint64_t v[22] = {t.scan,     (nchunks + 1) * sizeof(uint64_t), t.areas,    t.reg.areas,
                            t.dummy,    t.dummy_bytes,                    t.state,    t.state_bytes,
                            t.fields,   t.fields_bytes,                   t.njobs,    4,
                            t.jobs,     t.jobs_bytes,                     t.area_sz,  nchunks * 4,
                            t.job_cnt,  nchunks * 4,                      t.area_off, (nchunks + 1) * 8,
                            t.job_off,  (nchunks + 1) * 8};
    std::copy(v, v + 22, out);
    out[22] = t.total;
    return LZH_OK;
}

int lzh_debug_zstd_ragged_split_compact_slots(const uint64_t* out_sizes, size_t nchunks, size_t max_chunk_bytes,
                                              size_t total_out_bytes, uint64_t* area_off, uint64_t* job_off,
                                              uint8_t* in_split) {
    const ZstdRaggedSplitCompactTemp t = zstd_ragged_split_compact_temp(total_out_bytes, max_chunk_bytes, nchunks);
    // (the areas stand for the staging slots, the job counts for the record slots)
    return compact_slots_mirror(t.ok, LzhCompactRegions{t.reg.areas, t.reg.jobs}, out_sizes, nchunks, max_chunk_bytes,
                                area_off, job_off, in_split, [](uint64_t n) {
                                    const LzhZsplitRegions z = lzh_zstd_split_compact_slot(n);
                                    return LzhCompactRegions{z.areas, z.jobs};
                                });
}

// ---- 3g. the ragged split decoder in that layout: zstd_ragged_split_compact_temp is the sizing answer and what
// the launch is handed; 3c's contract, with the promised total.  Below the compact answer (or where there is none)
// every frame decodes in the one-wave kernel ----
size_t lzh_zstd_ragged_decompress_split_compact_temp_bytes(size_t total_out_bytes, size_t max_chunk_bytes,
                                                           size_t nchunks) {
    return zstd_ragged_split_compact_temp(total_out_bytes, max_chunk_bytes, nchunks).total;
}

int lzh_zstd_decompress_ragged_split_compact_async(const void* d_packed, size_t packed_readable, const uint32_t* d_csizes,
                                                   const uint64_t* d_offsets, void* const* d_out_ptrs,
                                                   const uint64_t* d_out_bytes, size_t nchunks, size_t max_chunk_bytes,
                                                   size_t total_out_bytes, int32_t* d_status, void* d_temp,
                                                   size_t temp_bytes, void* hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    return ragged_decompress(
        max_chunk_bytes <= kLz4SplitMax, nchunks, 1, ragged_decode_temp(nchunks),
        d_packed && d_csizes && d_out_ptrs && d_out_bytes && d_status && d_temp, d_csizes, d_offsets, d_temp, temp_bytes, s,
        [&](const uint64_t* offs, const DecodeTemp&) {
            const ZstdRaggedSplitCompactTemp z = zstd_ragged_split_compact_temp(total_out_bytes, max_chunk_bytes, nchunks);
            uint8_t* base = (uint8_t*)d_temp;
            if (z.ok && temp_bytes >= z.total) {
                const LzhZstdSplitCompactTemp T = {
                    base + z.areas, base + z.dummy, (int32_t*)(base + z.state), base + z.fields,
                    (uint32_t*)(base + z.njobs), base + z.jobs,
                    {(uint32_t*)(base + z.area_sz), (uint32_t*)(base + z.job_cnt), (uint64_t*)(base + z.area_off),
                     (uint64_t*)(base + z.job_off), z.reg.areas, z.reg.jobs}};
                return lzh_launch_zstd_decompress_ragged_split_compact((const uint8_t*)d_packed, packed_readable, offs,
                                                                       d_csizes, d_out_ptrs, d_out_bytes, max_chunk_bytes,
                                                                       d_status, (uint32_t)nchunks, T, s);
            }
            return lzh_launch_zstd_decompress_ragged((const uint8_t*)d_packed, packed_readable, offs, d_csizes, d_out_ptrs,
                                                     d_out_bytes, max_chunk_bytes, d_status, (uint32_t)nchunks, s);
        });
}

// ---- 3b, compact compress layout: every chunk's slots sized from its own size (ragged_slots.h); compact_temp
// lays the temp out for the sizing call, the async call and the debug calls ----
size_t lzh_ragged_compact_compress_temp_bytes(int codec, size_t total_in_bytes, size_t max_chunk_bytes, size_t nchunks) {
    if (!ragged_ok(codec, max_chunk_bytes)) return 0;
    return compact_temp(codec, total_in_bytes, max_chunk_bytes, nchunks).total;
}

int lzh_debug_ragged_compact_regions(int codec, size_t total_in_bytes, size_t max_chunk_bytes, size_t nchunks,
                                     uint64_t* out) {
    return compact_regions_out(ragged_ok(codec, max_chunk_bytes),
                               compact_temp(codec, total_in_bytes, max_chunk_bytes, nchunks), out);
}

int lzh_debug_ragged_compact_slots(int codec, const uint64_t* sizes, size_t nchunks, size_t max_chunk_bytes,
                                   size_t total_in_bytes, uint64_t* stage_off, uint64_t* rec_off, uint8_t* processed) {
    return compact_slots_mirror(ragged_ok(codec, max_chunk_bytes),
                                lzh_compact_regions(codec, total_in_bytes, max_chunk_bytes, nchunks), sizes, nchunks,
                                max_chunk_bytes, stage_off, rec_off, processed, [&](uint64_t n) {
                                    return LzhCompactRegions{lzh_slot_stage_bytes(codec, n),
                                                             lzh_slot_rec_bytes(codec, n, max_chunk_bytes > 65536)};
                                });
}

int lzh_compress_ragged_compact_async(int codec, int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                      size_t nchunks, size_t max_chunk_bytes, size_t total_in_bytes, void* d_packed,
                                      size_t packed_cap, uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp,
                                      size_t temp_bytes, void* hip_stream) {
    return ragged_compress(ragged_ok(codec, max_chunk_bytes), true, lzh_snappy_ragged_frags(max_chunk_bytes),
                           compact_temp(codec, total_in_bytes, max_chunk_bytes, nchunks), d_in_ptrs, d_in_bytes, nchunks,
                           max_chunk_bytes, d_packed, packed_cap, d_csizes, d_offsets, d_temp, temp_bytes, hip_stream,
                           [&](const LzhBatch& B, const LzhCompactSlots& S, hipStream_t s) {
                               const hipError_t e = lzh_launch_compact_slots(codec, B, S.L, s);
                               if (e != hipSuccess) return e;
                               return codec == LZH_CODEC_LZ4 ? lzh_launch_lz4_compact(B, level < 1 ? 1 : level, S, d_csizes, s)
                                                             : lzh_launch_snappy_compact(B, S, d_csizes, s);
                           });
}

// ---- 3c, compact compress layout: every chunk's staging slot and scratch slot sized from its own size and the
// level (zstd_ragged_slots.h); zstd_compact_temp lays the temp out for the sizing call, the async call and the
// debug calls ----
size_t lzh_zstd_ragged_compact_compress_temp_bytes(int level, size_t total_in_bytes, size_t max_chunk_bytes,
                                                   size_t nchunks) {
    if (!zstd_ragged_ok(level, max_chunk_bytes)) return 0;
    return zstd_compact_temp(level, total_in_bytes, max_chunk_bytes, nchunks).total;
}

int lzh_debug_zstd_ragged_compact_regions(int level, size_t total_in_bytes, size_t max_chunk_bytes, size_t nchunks,
                                          uint64_t* out) {
    return compact_regions_out(zstd_ragged_ok(level, max_chunk_bytes),
                               zstd_compact_temp(level, total_in_bytes, max_chunk_bytes, nchunks), out);
}

int lzh_debug_zstd_ragged_compact_slots(int level, const uint64_t* sizes, size_t nchunks, size_t max_chunk_bytes,
                                        size_t total_in_bytes, uint64_t* stage_off, uint64_t* scratch_off,
                                        uint8_t* processed) {
    return compact_slots_mirror(zstd_ragged_ok(level, max_chunk_bytes),
                                lzh_zstd_compact_regions(level, total_in_bytes, max_chunk_bytes, nchunks), sizes, nchunks,
                                max_chunk_bytes, stage_off, scratch_off, processed,
                                [&](uint64_t n) { return lzh_zstd_compact_slot(level, n); });
}

int lzh_zstd_compress_ragged_compact_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                           size_t nchunks, size_t max_chunk_bytes, size_t total_in_bytes,
                                           void* d_packed, size_t packed_cap, uint32_t* d_csizes, uint64_t* d_offsets,
                                           void* d_temp, size_t temp_bytes, void* hip_stream) {
    // (the layout's record fields carry the scratch slots: the pack kernel's lookup is the LZ4 / snappy one)
    return ragged_compress(zstd_ragged_ok(level, max_chunk_bytes), true, 1,
                           zstd_compact_temp(level, total_in_bytes, max_chunk_bytes, nchunks), d_in_ptrs, d_in_bytes, nchunks,
                           max_chunk_bytes, d_packed, packed_cap, d_csizes, d_offsets, d_temp, temp_bytes, hip_stream,
                           [&](const LzhBatch& B, const LzhCompactSlots& S, hipStream_t s) {
                               return lzh_launch_zstd_compact(B, level, S, d_csizes, s);
                           });
}

// ---- 3e. ragged zstd level-3 batches (the double-fast strategy): entry points of their own -- the calls of 3b keep
// refusing the codec and those of 3c the level -- through the skeleton of 3c; zstd_dfast_ragged_temp and
// zstd_dfast_compact_temp lay the temp out for the sizing calls, the async calls and the debug calls.  The frames
// decode with lzh_zstd_decompress_ragged_async ----
static bool zstd_dfast_ragged_ok(int level, size_t max_chunk_bytes) {
    return level == 3 && max_chunk_bytes <= kLz4SplitMax;
}

size_t lzh_zstd_dfast_ragged_compress_temp_bytes(int level, size_t max_chunk_bytes, size_t nchunks) {
    return zstd_dfast_ragged_ok(level, max_chunk_bytes) ? zstd_dfast_ragged_temp(nchunks, max_chunk_bytes).total : 0;
}

int lzh_zstd_dfast_compress_ragged_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                         size_t nchunks, size_t max_chunk_bytes, void* d_packed, size_t packed_cap,
                                         uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp, size_t temp_bytes,
                                         void* hip_stream) {
    return ragged_compress(zstd_dfast_ragged_ok(level, max_chunk_bytes), true, 1,
                           zstd_dfast_ragged_temp(nchunks, max_chunk_bytes), d_in_ptrs, d_in_bytes, nchunks, max_chunk_bytes,
                           d_packed, packed_cap, d_csizes, d_offsets, d_temp, temp_bytes, hip_stream,
                           [&](const LzhBatch& B, const LzhSlots& S, hipStream_t s) {
                               return lzh_launch_zstd_dfast_ragged(B, level, S, d_csizes, s);
                           });
}

size_t lzh_zstd_dfast_ragged_compact_compress_temp_bytes(int level, size_t total_in_bytes, size_t max_chunk_bytes,
                                                         size_t nchunks) {
    if (!zstd_dfast_ragged_ok(level, max_chunk_bytes)) return 0;
    return zstd_dfast_compact_temp(total_in_bytes, max_chunk_bytes, nchunks).total;
}

int lzh_debug_zstd_dfast_ragged_compact_regions(int level, size_t total_in_bytes, size_t max_chunk_bytes,
                                                size_t nchunks, uint64_t* out) {
    return compact_regions_out(zstd_dfast_ragged_ok(level, max_chunk_bytes),
                               zstd_dfast_compact_temp(total_in_bytes, max_chunk_bytes, nchunks), out);
}

int lzh_debug_zstd_dfast_ragged_compact_slots(int level, const uint64_t* sizes, size_t nchunks, size_t max_chunk_bytes,
                                              size_t total_in_bytes, uint64_t* stage_off, uint64_t* scratch_off,
                                              uint8_t* processed) {
    return compact_slots_mirror(zstd_dfast_ragged_ok(level, max_chunk_bytes),
                                lzh_zstd_dfast_compact_regions(total_in_bytes, max_chunk_bytes, nchunks), sizes, nchunks,
                                max_chunk_bytes, stage_off, scratch_off, processed,
                                [&](uint64_t n) { return lzh_zstd_dfast_compact_slot(n); });
}

int lzh_zstd_dfast_compress_ragged_compact_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                                 size_t nchunks, size_t max_chunk_bytes, size_t total_in_bytes,
                                                 void* d_packed, size_t packed_cap, uint32_t* d_csizes,
                                                 uint64_t* d_offsets, void* d_temp, size_t temp_bytes, void* hip_stream) {
    return ragged_compress(zstd_dfast_ragged_ok(level, max_chunk_bytes), true, 1,
                           zstd_dfast_compact_temp(total_in_bytes, max_chunk_bytes, nchunks), d_in_ptrs, d_in_bytes, nchunks,
                           max_chunk_bytes, d_packed, packed_cap, d_csizes, d_offsets, d_temp, temp_bytes, hip_stream,
                           [&](const LzhBatch& B, const LzhCompactSlots& S, hipStream_t s) {
                               return lzh_launch_zstd_dfast_compact(B, level, S, d_csizes, s);
                           });
}

// ---- 3i. ragged LZ4 frames: entry points of their own (the calls of 3b keep refusing both framed codecs), through
// the skeleton of 3b; lz4f_ragged_temp and lz4f_ragged_decode_temp lay the temp out for the sizing calls and the
// async calls.  Independent blocks alone: a level with LZH_LZ4F_LINKED is refused ----
static bool lz4f_ragged_ok(int level, size_t max_chunk_bytes) {
    return frame_level_ok(LZH_CODEC_LZ4F, level) && !(level & LZH_LZ4F_LINKED) && max_chunk_bytes <= kLz4SplitMax;
}
static Lz4fRaggedTemp lz4f_ragged_call_temp(int level, size_t max_chunk_bytes, size_t nchunks) {
    return lz4f_ragged_temp(level, frame_block_bytes(LZH_CODEC_LZ4F, level), max_chunk_bytes, nchunks);
}

size_t lzh_lz4f_ragged_compress_temp_bytes(int level, size_t max_chunk_bytes, size_t nchunks) {
    return lz4f_ragged_ok(level, max_chunk_bytes) ? lz4f_ragged_call_temp(level, max_chunk_bytes, nchunks).total : 0;
}

size_t lzh_lz4f_ragged_decompress_temp_bytes(size_t max_chunk_bytes, size_t nchunks) {
    return max_chunk_bytes <= kLz4SplitMax ? lz4f_ragged_decode_temp(nchunks, max_chunk_bytes).total : 0;
}

size_t lzh_lz4f_ragged_max_packed_bytes(size_t total_in_bytes, size_t nchunks) {
    // the sum of codec_bound over the chunks, whatever their sizes: 8 bytes per 64 KiB block (a chunk of s bytes has
    // ceil(s / 64 KiB) at the most, summed: total / 64 KiB + nchunks) and codec_bound(0) per chunk; then the uniform
    // call's 8 bytes per chunk and 64
    return total_in_bytes + 8 * (total_in_bytes / 65536 + nchunks) + nchunks * (codec_bound(LZH_CODEC_LZ4F, 0) + 8) + 64;
}

int lzh_lz4f_compress_ragged_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t nchunks,
                                   size_t max_chunk_bytes, void* d_packed, size_t packed_cap, uint32_t* d_csizes,
                                   uint64_t* d_offsets, void* d_temp, size_t temp_bytes, void* hip_stream) {
    const bool ok = lz4f_ragged_ok(level, max_chunk_bytes);
    const Lz4fRaggedTemp t = ok ? lz4f_ragged_call_temp(level, max_chunk_bytes, nchunks) : Lz4fRaggedTemp{};
    return ragged_compress(ok, true, t.g.bpf, t, d_in_ptrs, d_in_bytes, nchunks, max_chunk_bytes, d_packed, packed_cap,
                           d_csizes, d_offsets, d_temp, temp_bytes, hip_stream,
                           [&](const LzhBatch& B, const LzhRaggedFrame& R, hipStream_t s) {
                               return lzh_launch_lz4f_ragged(B, std::max(1, (level >> 8) & 0xff), R, d_csizes, s);
                           });
}

int lzh_lz4f_decompress_ragged_async(const void* d_packed, size_t packed_readable, const uint32_t* d_csizes,
                                     const uint64_t* d_offsets, void* const* d_out_ptrs, const uint64_t* d_out_bytes,
                                     size_t nchunks, size_t max_chunk_bytes, int32_t* d_status, void* d_temp,
                                     size_t temp_bytes, void* hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    const bool ok = max_chunk_bytes <= kLz4SplitMax;
    const uint32_t mb = ok ? frame_maxbpf(LZH_CODEC_LZ4F, max_chunk_bytes) : 1;
    return ragged_decompress(
        ok, nchunks, mb, ok ? lz4f_ragged_decode_temp(nchunks, max_chunk_bytes) : DecodeTemp{},
        d_packed && d_csizes && d_out_ptrs && d_out_bytes && d_status && d_temp, d_csizes, d_offsets, d_temp, temp_bytes, s,
        [&](const uint64_t* offs, const DecodeTemp& t) {
            uint8_t* base = (uint8_t*)d_temp;
            return lzh_launch_lz4f_decompress_ragged((const uint8_t*)d_packed, packed_readable, offs, d_csizes, d_out_ptrs,
                                                     d_out_bytes, max_chunk_bytes, d_status, (uint32_t)nchunks, mb,
                                                     base + t.desc, (int32_t*)(base + t.bstat),
                                                     (int32_t*)(base + t.fstat), s);
        });
}

}  // extern "C"

// ======================================================================= host layer

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = align_up(bytes + 4096, 1 << 20);
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; (void)hipGetLastError(); return -1; }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// the calling thread's current device is restored on every exit path of a row function
// (lzbench's process -- or a torch rank -- keeps allocating on the device it selected)
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

struct Dev {
    int id = 0;
    hipStream_t s = nullptr;      // kernels (even sub-batches)
    hipStream_t s2 = nullptr;     // kernels (odd sub-batches: overlaps the tail of the previous grid)
    hipStream_t sin = nullptr;    // host -> device copies
    hipStream_t sout = nullptr;   // device -> host copies
    DevBuf in, packed, temp, temp2, csizes, offsets, status;
    uint32_t* h_cs = nullptr;     // pinned: chunk sizes / statuses read back per sub-batch
    size_t h_cap = 0;
    int ensure_host(size_t n) {
        if (n <= h_cap) return 0;
        if (h_cs) (void)hipHostFree(h_cs);
        h_cs = nullptr;
        h_cap = 0;
        if (hipHostMalloc((void**)&h_cs, std::max<size_t>(n, 1024) * 4, hipHostMallocDefault) != hipSuccess) return -1;
        h_cap = std::max<size_t>(n, 1024);
        return 0;
    }
};

struct HostReg { void* p; size_t n; };

struct LzhCtx {
    uint32_t magic = 0x4c5a4858;  // "LZHX"
    int codec = 0;
    size_t chunk_size = 0;
    std::vector<Dev> devs;        // logical shards (may outnumber the physical devices)
    std::vector<HostReg> regs;    // host ranges page-locked by this row (lzbench reuses its buffers)
};

LzhCtx* ctx_of(char* wm) {
    LzhCtx* c = (LzhCtx*)wm;
    return (c && c->magic == 0x4c5a4858) ? c : nullptr;
}

// page-lock [p, p+n) once per row so the copies run at PCIe rate and asynchronously (the
// reference driver hands over pageable malloc'd buffers, lzbench.cpp:256-263); a range that
// cannot be registered is simply copied from pageable memory
void ensure_pinned(LzhCtx* c, const void* p, size_t n) {
    if (!p || n < (1u << 20)) return;
    const uintptr_t a0 = (uintptr_t)p & ~(uintptr_t)4095, a1 = ((uintptr_t)p + n + 4095) & ~(uintptr_t)4095;
    for (const HostReg& r : c->regs)
        if ((uintptr_t)r.p <= a0 && a1 <= (uintptr_t)r.p + r.n) return;
    if (hipHostRegister((void*)a0, a1 - a0, hipHostRegisterPortable) == hipSuccess) c->regs.push_back({(void*)a0, a1 - a0});
    else (void)hipGetLastError();
}

void ctx_free(LzhCtx* c) {
    DeviceGuard guard;
    for (Dev& d : c->devs) {
        (void)hipSetDevice(d.id);
        d.in.release(); d.packed.release(); d.temp.release(); d.temp2.release(); d.csizes.release(); d.offsets.release();
        d.status.release();
        if (d.h_cs) (void)hipHostFree(d.h_cs);
        if (d.s) (void)hipStreamDestroy(d.s);
        if (d.s2) (void)hipStreamDestroy(d.s2);
        if (d.sin) (void)hipStreamDestroy(d.sin);
        if (d.sout) (void)hipStreamDestroy(d.sout);
    }
    for (const HostReg& r : c->regs) (void)hipHostUnregister(r.p);
    c->magic = 0;
    delete c;
}

// ngpus logical shards (lzbench's additional_param of the row) starting at the caller's current
// device; shard g runs on device (current + g) mod count, so ngpus larger than the visible device
// count is legal (several shards share a device on their own streams; results are identical)
char* ctx_new(int codec, size_t chunk_size, size_t ngpus) {
    DeviceGuard guard;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        fprintf(stderr, "lzbench_hip: no HIP device available\n");
        return nullptr;
    }
    if (ngpus == 0) ngpus = 1;
    if (ngpus > 64) ngpus = 64;
    const int base = guard.prev >= 0 ? guard.prev : 0;
    LzhCtx* c = new LzhCtx();
    c->codec = codec;
    c->chunk_size = chunk_size;
    c->devs.resize(ngpus);
    for (size_t g = 0; g < ngpus; g++) {
        Dev& d = c->devs[g];
        d.id = (int)((base + g) % (size_t)count);
        if (hipSetDevice(d.id) != hipSuccess || hipStreamCreateWithFlags(&d.s, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&d.s2, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&d.sin, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&d.sout, hipStreamNonBlocking) != hipSuccess) {
            fprintf(stderr, "lzbench_hip: cannot open device %d\n", d.id);
            ctx_free(c);
            return nullptr;
        }
    }
    return (char*)c;
}

// chunks per pipelined sub-batch: ~128 MiB of input and at least 1 024 chunks (a full grid round
// of the widest-LDS kernel); consecutive sub-batches of a device alternate between two kernel
// streams so a grid's tail overlaps the next grid.  With several shards the sub-batch shrinks
// until every shard owns at least two.
size_t sub_batch_chunks(size_t chunk, size_t k, size_t G) {
    size_t sbk = std::max<size_t>(1024, ((size_t)128 << 20) / std::max<size_t>(chunk, 1));
    if (G > 1) sbk = std::min(sbk, std::max<size_t>(1, (k + 2 * G - 1) / (2 * G)));
    return sbk;
}

struct Events {
    std::vector<hipEvent_t> ev;
    hipEvent_t get(size_t i) {
        while (ev.size() <= i) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            ev.push_back(e);
        }
        return ev[i];
    }
    ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

// Sharding plan of one run (k chunks of `chunk` bytes covering n bytes): sub-batch j = chunks
// [j*sbk, min(k, (j+1)*sbk)) goes to shard j mod G as that shard's local slot j / G.  Every
// shard owns a contiguous set of index ranges, and the sub-batches finish roughly in index order
// across all shards, so the host gather (which must place sub-batch j after everything before
// it, lzbench.cpp:266-298 packing) can copy each one out as soon as its sizes land instead of
// waiting for whole shards in shard order.
struct Plan {
    size_t k, sbk, nsb, G;
    size_t chunk, n;
    size_t c_begin(size_t j) const { return j * sbk; }
    size_t c_count(size_t j) const { return std::min(sbk, k - j * sbk); }
    size_t b_begin(size_t j) const { return j * sbk * chunk; }
    size_t b_count(size_t j) const { return std::min(n, (j * sbk + c_count(j)) * chunk) - b_begin(j); }
    size_t shard(size_t j) const { return j % G; }
    size_t slot(size_t j) const { return j / G; }
    size_t slots(size_t g) const { return nsb > g ? (nsb - g + G - 1) / G : 0; }
};

// Host gather bookkeeping (pure host code, tested on the CPU through lzh_debug_gather_order):
// sub-batches finish in any order across the shards; sub-batch j's packed bytes go to the
// output at the sum of the packed sizes before it (lzbench.cpp:266-298), so j is placed as soon
// as its own sizes and every earlier sub-batch's are known -- the earliest moment its offset
// exists -- and the copies leave in chunk order.
struct GatherOrder {
    std::vector<uint8_t> done;
    std::vector<size_t> tot;
    size_t next = 0, base = 0;
    explicit GatherOrder(size_t n) : done(n, 0), tot(n, 0) {}
    bool finished() const { return next == done.size(); }
    // j's sizes are known (packed total t): place(j', offset) for every sub-batch that became placeable
    template <class F>
    int complete(size_t j, size_t t, F&& place) {
        done[j] = 1;
        tot[j] = t;
        while (next < done.size() && done[next]) {
            const int rc = place(next, base);
            if (rc) return rc;
            base += tot[next];
            next++;
        }
        return 0;
    }
};

// (a chunk size above the input is one chunk of the input's size: buffers are sized from the bytes
// present, not from lzbench's 1.79 GB default chunk)
size_t row_chunk(size_t n, size_t chunk) { return std::max<size_t>(std::min(chunk, n), 1); }

Plan make_plan(size_t ndev, size_t n, size_t chunk) {
    Plan p;
    p.n = n;
    p.chunk = chunk;
    p.k = lzh_num_chunks(n, chunk);
    p.G = std::max<size_t>(1, std::min(ndev, p.k));
    p.sbk = sub_batch_chunks(chunk, p.k, p.G);
    p.nsb = (p.k + p.sbk - 1) / p.sbk;
    p.G = std::min(p.G, p.nsb);
    return p;
}

// process one run: chunks [0, k) of uniform size `chunk` (last ragged) covering n bytes of
// host input; results appended at out (capacity outcap). Returns packed bytes, 0 when the
// packed output does not fit outcap, < 0 on error.  Per shard, sub-batches are pipelined over
// three streams (host->device copy | compress + scan + pack | device->host copy).
int64_t run_compress(LzhCtx* c, int level, const uint8_t* in, size_t n, size_t chunk, uint8_t* out, size_t outcap,
                     size_t* compr_sizes) {
    DeviceGuard guard;
    Range range("lzh:row_compress");
    chunk = row_chunk(n, chunk);
    const Plan P = make_plan(c->devs.size(), n, chunk);
    const size_t sb_in = std::min(n, P.sbk * chunk);                   // largest sub-batch input
    const size_t sb_packed = align_up(lzh_max_packed_bytes(c->codec, sb_in, chunk) + 64, 256);
    const size_t sb_temp = lzh_compress_temp_bytes(c->codec, sb_in, chunk);
    ensure_pinned(c, in, n);
    ensure_pinned(c, out, outcap);
    for (size_t g = 0; g < P.G; g++) {
        Dev& d = c->devs[g];
        const size_t m = P.slots(g);
        if (hipSetDevice(d.id) != hipSuccess) return LZH_EHIP;
        if (d.in.ensure(m * sb_in + 64) || d.packed.ensure(m * sb_packed) || d.temp.ensure(sb_temp) ||
            (m > 1 && d.temp2.ensure(sb_temp)) || d.csizes.ensure(m * P.sbk * 4 + 64) ||
            d.offsets.ensure(m * (P.sbk + 1) * 8 + 64) || d.ensure_host(m * P.sbk))
            return LZH_ESPACE;
    }
    Events evin, evk;
    for (size_t j = 0; j < P.nsb; j++) {     // issue every sub-batch, round-robin over the shards
        Dev& d = c->devs[P.shard(j)];
        const size_t l = P.slot(j), ck = P.c_count(j), rn = P.b_count(j);
        if (hipSetDevice(d.id) != hipSuccess) return LZH_EHIP;
        hipEvent_t e_in = evin.get(j), e_k = evk.get(j);
        if (!e_in || !e_k) return LZH_EHIP;
        uint8_t* din = (uint8_t*)d.in.p + l * sb_in;
        LZH_CHECK(hipMemcpyAsync(din, in + P.b_begin(j), rn, hipMemcpyHostToDevice, d.sin));
        hipStream_t ks = (l & 1) ? d.s2 : d.s;
        DevBuf& tb = (l & 1) ? d.temp2 : d.temp;
        LZH_CHECK(hipEventRecord(e_in, d.sin));
        LZH_CHECK(hipStreamWaitEvent(ks, e_in, 0));
        uint32_t* dcs = (uint32_t*)d.csizes.p + l * P.sbk;
        int rc = lzh_compress_async(c->codec, level, din, rn, rn + 64, chunk, (uint8_t*)d.packed.p + l * sb_packed,
                                    sb_packed, dcs, (uint64_t*)d.offsets.p + l * (P.sbk + 1), tb.p, tb.cap, ks);
        if (rc) return rc;
        LZH_CHECK(hipMemcpyAsync(d.h_cs + l * P.sbk, dcs, ck * 4, hipMemcpyDeviceToHost, ks));
        LZH_CHECK(hipEventRecord(e_k, ks));
    }
    // host-side gather: block on the next sub-batch in chunk order (its offset needs every earlier
    // one), then take any later sub-batch that has already finished on another shard without
    // waiting; copies leave as soon as their chunk-order offset is known
    bool fits = true;
    GatherOrder go(P.nsb);
    auto place = [&](size_t j, size_t base) -> int {
        Dev& d = c->devs[P.shard(j)];
        const size_t l = P.slot(j), tot = go.tot[j];
        if (!fits || base + tot > outcap) { fits = false; return 0; }   // lzbench: cannot store
        if (hipSetDevice(d.id) != hipSuccess) return LZH_EHIP;
        LZH_CHECK(hipStreamWaitEvent(d.sout, evk.get(j), 0));
        LZH_CHECK(hipMemcpyAsync(out + base, (uint8_t*)d.packed.p + l * sb_packed, tot, hipMemcpyDeviceToHost, d.sout));
        return 0;
    };
    auto take = [&](size_t j) -> int {   // j's kernels and size copy are done: record its sizes
        Dev& d = c->devs[P.shard(j)];
        const size_t l = P.slot(j), ck = P.c_count(j), c0 = P.c_begin(j);
        size_t tot = 0;
        const uint32_t* hs = d.h_cs + l * P.sbk;
        for (size_t i = 0; i < ck; i++) { compr_sizes[c0 + i] = hs[i]; tot += hs[i]; }
        return go.complete(j, tot, place);
    };
    while (!go.finished()) {
        const size_t j0 = go.next;
        hipError_t q = hipEventSynchronize(evk.get(j0));
        if (q != hipSuccess) {
            fprintf(stderr, "lzbench_hip: sub-batch %zu failed: %s\n", j0, hipGetErrorString(q));
            return LZH_EHIP;
        }
        if (const int rc = take(j0)) return rc;
        for (size_t j = go.next; j < P.nsb; j++) {
            if (go.done[j]) continue;
            q = hipEventQuery(evk.get(j));
            if (q == hipErrorNotReady) continue;
            if (q != hipSuccess) {
                fprintf(stderr, "lzbench_hip: sub-batch %zu failed: %s\n", j, hipGetErrorString(q));
                return LZH_EHIP;
            }
            if (const int rc = take(j)) return rc;
        }
    }
    const size_t base = go.base;
    for (size_t g = 0; g < P.G; g++) {
        if (hipSetDevice(c->devs[g].id) != hipSuccess || hipStreamSynchronize(c->devs[g].sout) != hipSuccess ||
            hipStreamSynchronize(c->devs[g].s) != hipSuccess || hipStreamSynchronize(c->devs[g].s2) != hipSuccess)
            return LZH_EHIP;
    }
    return fits ? (int64_t)base : 0;
}

// Inverse of run_compress over the same plan.  Returns the decoded byte count (== n) or < 0:
// a chunk whose decoder reports anything but its own size is malformed (LZH_ECORRUPT), which
// keeps lzbench's length check (lzbench.cpp:433-437) honest for short decodes.
int64_t run_decompress(LzhCtx* c, const uint8_t* in, const size_t* compr_sizes, size_t n, size_t chunk, uint8_t* out) {
    DeviceGuard guard;
    Range range("lzh:row_decompress");
    chunk = row_chunk(n, chunk);
    const Plan P = make_plan(c->devs.size(), n, chunk);
    const size_t k = P.k;
    std::vector<size_t> coff(k + 1, 0);
    for (size_t i = 0; i < k; i++) coff[i + 1] = coff[i] + compr_sizes[i];
    size_t sb_cin = 0;                        // largest compressed sub-batch
    for (size_t j = 0; j < P.nsb; j++)
        sb_cin = std::max(sb_cin, coff[P.c_begin(j) + P.c_count(j)] - coff[P.c_begin(j)]);
    sb_cin = align_up(sb_cin + 64, 256);
    const size_t sb_out = std::min(n, P.sbk * chunk);
    const size_t sb_temp = lzh_decompress_temp_bytes(c->codec, sb_out, chunk);
    ensure_pinned(c, in, coff[k]);
    ensure_pinned(c, out, n);
    for (size_t g = 0; g < P.G; g++) {
        Dev& d = c->devs[g];
        const size_t m = P.slots(g);
        if (hipSetDevice(d.id) != hipSuccess) return LZH_EHIP;
        if (d.in.ensure(m * sb_cin) || d.packed.ensure(m * sb_out + 64) || d.csizes.ensure(m * P.sbk * 4 + 64) ||
            d.status.ensure(m * P.sbk * 4 + 64) || d.temp.ensure(sb_temp) || d.temp2.ensure(sb_temp) ||
            d.ensure_host(2 * m * P.sbk))
            return LZH_ESPACE;
    }
    Events evin, evk;
    for (size_t j = 0; j < P.nsb; j++) {
        Dev& d = c->devs[P.shard(j)];
        const size_t l = P.slot(j), m = P.slots(P.shard(j)), ck = P.c_count(j), c0 = P.c_begin(j);
        const size_t rn = P.b_count(j), po = coff[c0], pn = coff[c0 + ck] - po;
        if (hipSetDevice(d.id) != hipSuccess) return LZH_EHIP;
        hipEvent_t e_in = evin.get(j), e_k = evk.get(j);
        if (!e_in || !e_k) return LZH_EHIP;
        uint32_t* h_in = d.h_cs + l * P.sbk;                  // sizes in
        for (size_t i = 0; i < ck; i++) h_in[i] = (uint32_t)compr_sizes[c0 + i];
        uint8_t* din = (uint8_t*)d.in.p + l * sb_cin;
        uint32_t* dcs = (uint32_t*)d.csizes.p + l * P.sbk;
        int32_t* dst = (int32_t*)d.status.p + l * P.sbk;
        uint8_t* dout = (uint8_t*)d.packed.p + l * sb_out;
        LZH_CHECK(hipMemcpyAsync(din, in + po, pn, hipMemcpyHostToDevice, d.sin));
        LZH_CHECK(hipMemcpyAsync(dcs, h_in, ck * 4, hipMemcpyHostToDevice, d.sin));
        LZH_CHECK(hipEventRecord(e_in, d.sin));
        hipStream_t ks = (l & 1) ? d.s2 : d.s;
        DevBuf& tb = (l & 1) ? d.temp2 : d.temp;
        LZH_CHECK(hipStreamWaitEvent(ks, e_in, 0));
        int rc = lzh_decompress_async(c->codec, din, pn + 64, dcs, nullptr, rn, chunk, dout, dst, tb.p, tb.cap, ks);
        if (rc) return rc;
        LZH_CHECK(hipEventRecord(e_k, ks));
        LZH_CHECK(hipStreamWaitEvent(d.sout, e_k, 0));
        int32_t* h_st = (int32_t*)d.h_cs + m * P.sbk + l * P.sbk;   // statuses out
        LZH_CHECK(hipMemcpyAsync(h_st, dst, ck * 4, hipMemcpyDeviceToHost, d.sout));
        LZH_CHECK(hipMemcpyAsync(out + P.b_begin(j), dout, rn, hipMemcpyDeviceToHost, d.sout));
    }
    for (size_t g = 0; g < P.G; g++) {
        Dev& d = c->devs[g];
        if (hipSetDevice(d.id) != hipSuccess || hipStreamSynchronize(d.sout) != hipSuccess ||
            hipStreamSynchronize(d.s) != hipSuccess || hipStreamSynchronize(d.s2) != hipSuccess)
            return LZH_EHIP;
    }
    int64_t sum = 0;
    bool bad = false;
    for (size_t j = 0; j < P.nsb; j++) {
        const Dev& d = c->devs[P.shard(j)];
        const size_t l = P.slot(j), m = P.slots(P.shard(j)), ck = P.c_count(j), c0 = P.c_begin(j);
        const int32_t* h_st = (const int32_t*)d.h_cs + m * P.sbk + l * P.sbk;
        for (size_t i = 0; i < ck; i++) {
            const int64_t part = (int64_t)std::min(chunk, n - (c0 + i) * chunk);
            if (h_st[i] != part) bad = true;
            sum += h_st[i];
        }
    }
    return bad ? LZH_ECORRUPT : sum;
}

}  // namespace

// debug (CPU): the gather's placement order for sub-batches completing in `order` with packed
// sizes `sizes`: placed[i] = (sub-batch, offset, index into `order` of the completion that placed it)
extern "C" int lzh_debug_gather_order(size_t nsb, const uint64_t* order, const uint64_t* sizes, uint64_t* placed) {
    GatherOrder go(nsb);
    size_t np = 0, at = 0;
    for (size_t i = 0; i < nsb; i++) {
        at = i;
        go.complete((size_t)order[i], (size_t)sizes[order[i]], [&](size_t j, size_t base) {
            placed[3 * np] = j;
            placed[3 * np + 1] = base;
            placed[3 * np + 2] = at;
            np++;
            return 0;
        });
    }
    return (int)np;
}

extern "C" int lzh_debug_plan(size_t ngpus, size_t n, size_t chunk_size, int codec, uint64_t* out, int nout) {
    if (!out || nout <= 0 || chunk_size == 0) return 0;
    chunk_size = row_chunk(n, chunk_size);
    const Plan P = make_plan(std::max<size_t>(std::min<size_t>(ngpus, 64), 1), n, chunk_size);
    const size_t sb_in = std::min(n, P.sbk * chunk_size);
    std::vector<uint64_t> v = {P.k, P.sbk, P.nsb, P.G, sb_in,
                               align_up(lzh_max_packed_bytes(codec, sb_in, chunk_size) + 64, 256),
                               lzh_compress_temp_bytes(codec, sb_in, chunk_size)};
    for (size_t g = 0; g < P.G; g++) v.push_back(P.slots(g));
    const int m = std::min<int>(nout, (int)v.size());
    for (int i = 0; i < m; i++) out[i] = v[i];
    return m;
}

namespace {

int64_t one_chunk_compress(int codec_expect, char* in, size_t insize, char* out, size_t outsize, size_t level, char* wm) {
    LzhCtx* c = ctx_of(wm);
    if (!c || c->codec != codec_expect) return 0;
    size_t cs = 0;
    const size_t chunk = std::max<size_t>(insize, 1);
    int64_t r = run_compress(c, (int)level, (const uint8_t*)in, insize, chunk, (uint8_t*)out, outsize, &cs);
    return r <= 0 ? 0 : (int64_t)cs;
}

int64_t one_chunk_decompress(int codec_expect, char* in, size_t insize, char* out, size_t outsize, char* wm) {
    LzhCtx* c = ctx_of(wm);
    if (!c || c->codec != codec_expect) return 0;
    size_t cs = insize;
    const size_t chunk = std::max<size_t>(outsize, 1);
    return run_decompress(c, (const uint8_t*)in, &cs, outsize, chunk, (uint8_t*)out);
}

}  // namespace

extern "C" {

char* lzbench_hip_lz4_init(size_t chunk_size, size_t level, size_t ngpus) { (void)level; return ctx_new(LZH_CODEC_LZ4, chunk_size, ngpus); }
char* lzbench_hip_snappy_init(size_t chunk_size, size_t level, size_t ngpus) { (void)level; return ctx_new(LZH_CODEC_SNAPPY, chunk_size, ngpus); }
char* lzbench_hip_memcpy_init(size_t chunk_size, size_t level, size_t ngpus) { (void)level; return ctx_new(LZH_CODEC_MEMCPY, chunk_size, ngpus); }
char* lzbench_hip_zstd_init(size_t chunk_size, size_t level, size_t ngpus) { (void)level; return ctx_new(LZH_CODEC_ZSTD, chunk_size, ngpus); }
char* lzbench_hip_zstd_dfast_init(size_t chunk_size, size_t level, size_t ngpus) { (void)level; return ctx_new(LZH_CODEC_ZSTD_DFAST, chunk_size, ngpus); }
char* lzbench_hip_lz4frame_init(size_t chunk_size, size_t level, size_t ngpus) { (void)level; return ctx_new(LZH_CODEC_LZ4F, chunk_size, ngpus); }
char* lzbench_hip_nvcomp_lz4_init(size_t chunk_size, size_t level, size_t ngpus) { (void)level; return ctx_new(LZH_CODEC_NVLZ4, chunk_size, ngpus); }

void lzbench_hip_deinit(char* wm) {
    LzhCtx* c = ctx_of(wm);
    if (c) ctx_free(c);
}

int64_t lzbench_hip_lz4_compress(char* in, size_t insize, char* out, size_t outsize, size_t, size_t, char* wm) {
    return one_chunk_compress(LZH_CODEC_LZ4, in, insize, out, outsize, 1, wm);
}
int64_t lzbench_hip_lz4fast_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t, char* wm) {
    return one_chunk_compress(LZH_CODEC_LZ4, in, insize, out, outsize, level, wm);
}
int64_t lzbench_hip_lz4_decompress(char* in, size_t insize, char* out, size_t outsize, size_t, size_t, char* wm) {
    return one_chunk_decompress(LZH_CODEC_LZ4, in, insize, out, outsize, wm);
}
int64_t lzbench_hip_snappy_compress(char* in, size_t insize, char* out, size_t outsize, size_t, size_t, char* wm) {
    return one_chunk_compress(LZH_CODEC_SNAPPY, in, insize, out, outsize, 0, wm);
}
int64_t lzbench_hip_snappy_decompress(char* in, size_t insize, char* out, size_t outsize, size_t, size_t, char* wm) {
    return one_chunk_decompress(LZH_CODEC_SNAPPY, in, insize, out, outsize, wm);
}
int64_t lzbench_hip_zstd_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t, char* wm) {
    return one_chunk_compress(LZH_CODEC_ZSTD, in, insize, out, outsize, level, wm);
}
int64_t lzbench_hip_zstd_decompress(char* in, size_t insize, char* out, size_t outsize, size_t, size_t, char* wm) {
    // (a workmem of either zstd init: the level-3 codec writes the same frames)
    const LzhCtx* c = ctx_of(wm);
    const int codec = c && c->codec == LZH_CODEC_ZSTD_DFAST ? LZH_CODEC_ZSTD_DFAST : LZH_CODEC_ZSTD;
    return one_chunk_decompress(codec, in, insize, out, outsize, wm);
}
int64_t lzbench_hip_zstd_dfast_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t, char* wm) {
    return one_chunk_compress(LZH_CODEC_ZSTD_DFAST, in, insize, out, outsize, level, wm);
}
int64_t lzbench_hip_lz4frame_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t, char* wm) {
    return one_chunk_compress(LZH_CODEC_LZ4F, in, insize, out, outsize, level, wm);
}
int64_t lzbench_hip_lz4frame_decompress(char* in, size_t insize, char* out, size_t outsize, size_t, size_t, char* wm) {
    return one_chunk_decompress(LZH_CODEC_LZ4F, in, insize, out, outsize, wm);
}
int64_t lzbench_hip_nvcomp_lz4_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t, char* wm) {
    return one_chunk_compress(LZH_CODEC_NVLZ4, in, insize, out, outsize, level, wm);
}
int64_t lzbench_hip_nvcomp_lz4_decompress(char* in, size_t insize, char* out, size_t outsize, size_t, size_t, char* wm) {
    return one_chunk_decompress(LZH_CODEC_NVLZ4, in, insize, out, outsize, wm);
}
int64_t lzbench_hip_memcpy(char* in, size_t insize, char* out, size_t outsize, size_t, size_t, char* wm) {
    LzhCtx* c = ctx_of(wm);
    if (!c || outsize < insize) return 0;
    DeviceGuard guard;
    Dev& d = c->devs[0];
    if (hipSetDevice(d.id) != hipSuccess || d.in.ensure(insize + 64)) return 0;
    ensure_pinned(c, in, insize);
    ensure_pinned(c, out, outsize);
    if (hipMemcpyAsync(d.in.p, in, insize, hipMemcpyHostToDevice, d.s) != hipSuccess ||
        hipMemcpyAsync(out, d.in.p, insize, hipMemcpyDeviceToHost, d.s) != hipSuccess ||
        hipStreamSynchronize(d.s) != hipSuccess)
        return 0;
    return (int64_t)insize;
}

int64_t lzbench_hip_compress_batch(const char* in, const size_t* chunk_sizes, int nchunks, char* out, size_t outcap,
                                   size_t* compr_sizes, size_t level, size_t, char* wm) {
    LzhCtx* c = ctx_of(wm);
    if (!c || nchunks < 0) return 0;
    // runs of uniform chunking: a run ends after a chunk shorter than the first of the run
    int64_t total = 0;
    size_t ipos = 0;
    int i = 0;
    while (i < nchunks) {
        const size_t chunk = chunk_sizes[i];
        int j = i;
        size_t n = 0;
        while (j < nchunks && chunk_sizes[j] <= chunk) {
            n += chunk_sizes[j];
            if (chunk_sizes[j++] < chunk) break;
        }
        int64_t r = run_compress(c, (int)level, (const uint8_t*)in + ipos, n, std::max<size_t>(chunk, 1),
                                 (uint8_t*)out + total, outcap - (size_t)total, compr_sizes + i);
        if (r <= 0 && n > 0) return r;
        total += r;
        ipos += n;
        i = j;
    }
    return total;
}

int64_t lzbench_hip_decompress_batch(const char* in, const size_t* compr_sizes, const size_t* chunk_sizes, int nchunks,
                                     char* out, size_t outcap, size_t, size_t, char* wm) {
    LzhCtx* c = ctx_of(wm);
    if (!c || nchunks < 0) return 0;
    int64_t total = 0;
    size_t ipos = 0;
    int i = 0;
    while (i < nchunks) {
        const size_t chunk = chunk_sizes[i];
        int j = i;
        size_t n = 0, cn = 0;
        while (j < nchunks && chunk_sizes[j] <= chunk) {
            n += chunk_sizes[j];
            cn += compr_sizes[j];
            if (chunk_sizes[j++] < chunk) break;
        }
        if ((size_t)total + n > outcap) return 0;
        int64_t r = run_decompress(c, (const uint8_t*)in + ipos, compr_sizes + i, n, std::max<size_t>(chunk, 1),
                                   (uint8_t*)out + total);
        if (r < 0) return r;
        total += (int64_t)n;
        ipos += cn;
        i = j;
    }
    return total;
}

}  // extern "C"
