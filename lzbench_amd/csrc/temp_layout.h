// lzbench_amd/csrc/temp_layout.h -- where everything lives in the caller's d_temp (host only, for api.cpp).
//
// Every call of the device API carves its temp buffer with one of the functions below, and the matching
// *_temp_bytes function returns the same struct's `total`: the size promised to the caller and the offsets the
// kernels are handed cannot disagree.  A layout is built with a TempCursor, so its regions are disjoint, in the
// order they are taken, and each starts at a multiple of 256.  The spare 256 bytes after most regions (kGap) are
// part of the published sizes (tests/golden/sizing.json) and addressed by nobody.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/lzbench_hip.h"
#include "launch.h"
#include "ragged_slots.h"

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// LZ4 / snappy chunks up to this size compress in two kernels (parse -> 8-byte sequence records -> emit);
// larger ones (24-bit record fields) in the single kernel that assembles the block itself
static const size_t kLz4SplitMax = (size_t)16 << 20;

struct TempCursor {
    size_t at = 0;
    // the offset of the next region: `bytes` rounded up to 256, then `gap` spare bytes
    size_t take(size_t bytes, size_t gap = 0) { return take_sized(align_up(bytes, 256) + gap); }
    // a region whose size another file computes for its own carving (zstdc_hip.hip, decode_hip.hip): as it is
    size_t take_sized(size_t bytes) { const size_t o = at; at += bytes; return o; }
};
static const size_t kGap = 256;

// ---- compression of k chunks of up to `chunk` bytes (uniform calls: k = lzh_num_chunks(n, chunk); ragged
// uniform-slot batches: k = nchunks, chunk = max_chunk_bytes):
//   k staging slots of `stride` | split (LZ4 / snappy up to kLz4SplitMax): k record slots of `rec_stride` at
//   `recs`, then the per-chunk record counts at `hdr` (LZ4: 8 bytes a chunk; snappy: a u32 per fragment)
//                               | zstd: k per-frame scratch areas of the two zstd kernels at `recs`, worst level
//                               | zstd level 3 (LZH_CODEC_ZSTD_DFAST): the same with that codec's own scratch stride
// per-frame scratch of the level-3 codec: the fast levels' areas below the table (the zstd kernels' Layout), then
// the long and the short table, each the largest of any chunk size up to `chunk` (zstdc_dfast_hip.hip computes it)
static inline size_t zstd_dfast_scratch_stride(size_t chunk) { return lzh_zstd_dfast_scratch_stride(chunk); }

struct ChunkTemp {
    bool split;
    size_t stride, rec_stride, stage, recs, hdr, total;
    LzhSlots slots(uint8_t* base) const {   // (the launchers' bundle; record counts only where there are records)
        return {base + stage, stride, base + recs, rec_stride, split ? (uint32_t*)(base + hdr) : nullptr};
    }
};
static inline ChunkTemp chunk_temp(int codec, size_t k, size_t chunk) {
    ChunkTemp t = {};
    TempCursor c;
    t.split = (codec == LZH_CODEC_LZ4 || codec == LZH_CODEC_SNAPPY) && chunk <= kLz4SplitMax;
    t.stride = lzh_stage_stride(codec, chunk);
    t.stage = c.take(k * t.stride, kGap);
    t.recs = t.hdr = c.at;
    if (t.split) {
        t.rec_stride = codec == LZH_CODEC_LZ4 ? lzh_lz4_rec_stride(chunk) : lzh_snappy_rec_stride(chunk);
        t.recs = c.take(k * t.rec_stride);
        t.hdr = c.take(codec == LZH_CODEC_LZ4 ? k * 8 : k * 4 * lzh_snappy_ragged_frags(chunk), kGap);
    } else if (codec == LZH_CODEC_ZSTD) {
        for (int lv : {1, 2, -1, -2}) t.rec_stride = std::max(t.rec_stride, lzh_zstd_scratch_stride(chunk, lv));
        t.recs = c.take_sized(k * t.rec_stride + kGap);
    } else if (codec == LZH_CODEC_ZSTD_DFAST) {
        t.rec_stride = zstd_dfast_scratch_stride(chunk);
        t.recs = c.take_sized(k * t.rec_stride + kGap);
    }
    t.total = c.at;
    return t;
}

// ---- LZ4 compression of k chunks of up to `chunk` bytes with a shared dictionary (3d): the staging slots of
// chunk_temp, then LZ4_loadDict's table (4096 u32).  No records (the parse emits in-kernel) and no copy of the
// dictionary: below chunk_temp(LZH_CODEC_LZ4, k, chunk) but for the table.
static const size_t kLz4DictMax = (size_t)4 << 20;      // largest chunk of the dictionary calls
struct DictTemp {
    size_t stride, stage, tab, total;
    LzhSlots slots(uint8_t* base) const { return {base + stage, stride, nullptr, 0, nullptr}; }
};
static inline DictTemp lz4_dict_temp(size_t k, size_t chunk) {
    DictTemp t;
    TempCursor c;
    t.stride = lzh_stage_stride(LZH_CODEC_LZ4, chunk);
    t.stage = c.take(k * t.stride, kGap);
    t.tab = c.take(4096 * sizeof(uint32_t), kGap);
    t.total = c.at;
    return t;
}

// ---- zstd compression of k chunks of up to `chunk` bytes with a shared dictionary (3f): the staging slots of
// chunk_temp(zstd), then k scratch areas of the dictionary calls' own stride (the zstd kernels' areas for a block of
// `chunk` bytes and the frame's copy of its class's table, the largest any frame of the batch can take), then the
// table region: one filled table per (hashLog, minMatch) class, a constant bound (lzh_zstd_dict_tables_bytes).
static const size_t kZstdDictMax = (size_t)131072;      // largest dictionary and largest chunk of the dictionary calls
struct ZstdDictTemp {
    size_t stride, rec_stride, stage, recs, tabs, total;
    LzhSlots slots(uint8_t* base) const { return {base + stage, stride, base + recs, rec_stride, nullptr}; }
};
static inline ZstdDictTemp zstd_dict_temp_with(size_t (*scratch_stride)(size_t, size_t), size_t (*tables_bytes)(void),
                                               size_t dict_bytes, size_t k, size_t chunk) {
    ZstdDictTemp t;
    TempCursor c;
    chunk = std::max<size_t>(chunk, 1);                 // (a batch of empty chunks is laid out as one of 1-byte chunks)
    t.stride = lzh_stage_stride(LZH_CODEC_ZSTD, chunk);
    t.rec_stride = scratch_stride(dict_bytes, chunk);
    t.stage = c.take(k * t.stride, kGap);
    t.recs = c.take(k * t.rec_stride, kGap);
    t.tabs = c.take(tables_bytes(), kGap);
    t.total = c.at;
    return t;
}
static inline ZstdDictTemp zstd_dict_temp(size_t dict_bytes, size_t k, size_t chunk) {
    return zstd_dict_temp_with(lzh_zstd_dict_scratch_stride, lzh_zstd_dict_tables_bytes, dict_bytes, k, chunk);
}

// ---- zstd level-3 compression of k chunks with a shared dictionary (3h): 3f's three regions with the level-3 calls'
// own strides -- the staging slots, k scratch areas (the zstd kernels' areas for a block of `chunk` bytes and the frame's
// private pair of tables, the largest any frame of the batch can take), the table region (one filled pair per class, a
// constant bound: lzh_zstd_dfast_dict_tables_bytes).
static inline ZstdDictTemp zstd_dfast_dict_temp(size_t dict_bytes, size_t k, size_t chunk) {
    return zstd_dict_temp_with(lzh_zstd_dfast_dict_scratch_stride, lzh_zstd_dfast_dict_tables_bytes, dict_bytes, k, chunk);
}

// ---- framed compression: frames of F bytes (the chunks) cut into blocks of bs = min(F, B) bytes:
//   staging slots | LZ4 sequence records of the blocks, then 8 bytes per block (linked frames: the per-frame
//   table snapshots instead) | block sizes | block offsets inside their frame
struct FrameGeo {
    size_t F, bs, nframes, nblocks;
    uint32_t bpf;
};
static inline FrameGeo frame_geo(size_t B, size_t n, size_t F) {
    FrameGeo g;
    g.F = F;
    g.bs = std::min(F, B);
    g.bpf = (uint32_t)((F + g.bs - 1) / g.bs);
    g.nframes = lzh_num_chunks(n, F);
    if (n == 0) {
        g.nblocks = 0;
    } else {
        const size_t last = n - (g.nframes - 1) * F;
        g.nblocks = (g.nframes - 1) * g.bpf + (last + g.bs - 1) / g.bs;
    }
    return g;
}

struct FrameTemp {
    size_t stride, rec_stride, stage, recs, hdr, bcs, rel, total;
    LzhFrameSlots slots(uint8_t* base) const {
        return {{base + stage, stride, base + recs, rec_stride, (uint32_t*)(base + hdr)}, (uint32_t*)(base + bcs),
                (uint32_t*)(base + rel)};
    }
};
static inline FrameTemp frame_temp(const FrameGeo& g) {
    FrameTemp t;
    TempCursor c;
    t.stride = lzh_stage_stride(LZH_CODEC_LZ4, g.bs);
    t.rec_stride = lzh_lz4_rec_stride(g.bs);
    t.stage = c.take(g.nblocks * t.stride, kGap);
    t.recs = c.take(g.nblocks * t.rec_stride);
    t.hdr = c.take(g.nblocks * 8, kGap);
    t.bcs = c.take(g.nblocks * 4, kGap);
    t.rel = c.take(g.nblocks * 4, kGap);
    t.total = c.at;
    return t;
}

// ---- ragged LZ4 frames (3i), uniform slots: every frame has the block slots of the largest chunk -- blocks of
// bs = min(B, max_bytes) bytes (B: the level's block size), bpf = ceil(max_bytes / bs) of them -- so the layout is
// frame_temp for nchunks * bpf blocks, then the derived block batch (a pointer and a size per block slot):
//   staging slots | LZ4 sequence records, 8 bytes per block | block sizes | block offsets | block pointers | block sizes
// (a batch of empty chunks is laid out with one 1-byte block slot per frame)
struct Lz4fRaggedTemp {
    FrameGeo g;
    FrameTemp f;
    size_t bptrs, bbytes, total;
    int params;
    LzhRaggedFrame slots(uint8_t* base) const {
        return {f.slots(base), (const void**)(base + bptrs), (uint64_t*)(base + bbytes), g.bs, g.bpf, params};
    }
};
static inline Lz4fRaggedTemp lz4f_ragged_temp(int params, size_t B, size_t max_bytes, size_t nchunks) {
    Lz4fRaggedTemp t;
    t.params = params;
    t.g.F = max_bytes;
    t.g.bs = std::max<size_t>(std::min(B, max_bytes), 1);
    t.g.bpf = (uint32_t)std::max<size_t>((max_bytes + t.g.bs - 1) / t.g.bs, 1);
    t.g.nframes = nchunks;
    t.g.nblocks = nchunks * t.g.bpf;
    t.f = frame_temp(t.g);
    TempCursor c;
    c.at = t.f.total;
    t.bptrs = c.take(t.g.nblocks * 8);
    t.bbytes = c.take(t.g.nblocks * 8, kGap);
    t.total = c.at;
    return t;
}

// ---- ragged compression, compact layout: every chunk's slots sized from its own size (LZ4 / snappy:
// ragged_slots.h; zstd: its own size and the call's level, zstd_ragged_slots.h, where the uniform-slot chunk_temp
// takes the worst of four levels):
//   staging region | record region (zstd: the scratch region, the two zstd kernels' per-frame areas)
//   | LZ4 / snappy: the per-chunk record counts (sized for max_bytes as in chunk_temp)
//   | staging-slot sizes | record-slot sizes (u32 each) | staging-slot offsets | record-slot offsets
//   (nchunks + 1 u64 each, scanned on the device)
// The spare 256 bytes differ: LZ4 / snappy have none after the records and one after the last array; zstd keeps
// chunk_temp's after both regions and its arrays follow without one, so its total never passes chunk_temp's for
// the same nchunks and max_bytes by more than the four arrays.
struct CompactTemp {
    LzhCompactRegions reg;
    size_t stage, recs, hdr, stage_sz, rec_sz, stage_off, rec_off, total;
    LzhCompactSlots slots(uint8_t* base) const {   // (hdr 0: a zstd layout, no record counts)
        return {base + stage, base + recs, hdr ? (uint32_t*)(base + hdr) : nullptr,
                {(uint32_t*)(base + stage_sz), (uint32_t*)(base + rec_sz), (uint64_t*)(base + stage_off),
                 (uint64_t*)(base + rec_off), reg.stage, reg.recs}};
    }
};
static inline void compact_arrays(CompactTemp& t, TempCursor& c, size_t nchunks, size_t gap) {
    t.stage_sz = c.take(nchunks * 4);
    t.rec_sz = c.take(nchunks * 4);
    t.stage_off = c.take((nchunks + 1) * 8);
    t.rec_off = c.take((nchunks + 1) * 8, gap);
    t.total = c.at;
}
static inline CompactTemp compact_temp(int codec, size_t total_in, size_t max_bytes, size_t nchunks) {
    CompactTemp t;
    TempCursor c;
    t.reg = lzh_compact_regions(codec, total_in, max_bytes, nchunks);
    t.stage = c.take(t.reg.stage, kGap);
    t.recs = c.take(t.reg.recs);
    t.hdr = c.take(codec == LZH_CODEC_LZ4 ? nchunks * 8 : nchunks * 4 * lzh_snappy_ragged_frags(max_bytes), kGap);
    compact_arrays(t, c, nchunks, kGap);
    return t;
}
static inline CompactTemp zstd_compact_temp(int level, size_t total_in, size_t max_bytes, size_t nchunks) {
    CompactTemp t = {};   // (no record counts: hdr stays 0)
    TempCursor c;
    t.reg = lzh_zstd_compact_regions(level, total_in, max_bytes, nchunks);
    t.stage = c.take(t.reg.stage, kGap);
    t.recs = c.take(t.reg.recs, kGap);
    compact_arrays(t, c, nchunks, 0);
    return t;
}

// ---- ragged zstd level-3 compression (3e), both layouts without spare bytes, so the published formulas are exact:
// uniform slots: k staging slots of lzh_stage_stride(LZH_CODEC_ZSTD, chunk) | k scratch areas of the level-3 stride
// (a batch of empty chunks is laid out as one of 1-byte chunks, as in 3c);
// compact: staging region | scratch region (zstd_dfast_slots.h) | the placement's four arrays -- each region at most
// k x the slot above, so the total never passes the uniform-slot one by more than the four arrays.
static inline ChunkTemp zstd_dfast_ragged_temp(size_t k, size_t chunk) {
    ChunkTemp t = {};
    TempCursor c;
    chunk = std::max<size_t>(chunk, 1);
    t.stride = lzh_stage_stride(LZH_CODEC_ZSTD, chunk);
    t.rec_stride = zstd_dfast_scratch_stride(chunk);
    t.stage = c.take(k * t.stride);
    t.recs = t.hdr = c.take(k * t.rec_stride);
    t.total = c.at;
    return t;
}
static inline CompactTemp zstd_dfast_compact_temp(size_t total_in, size_t max_bytes, size_t nchunks) {
    CompactTemp t = {};   // (no record counts: hdr stays 0)
    TempCursor c;
    t.reg = lzh_zstd_dfast_compact_regions(total_in, max_bytes, nchunks);
    t.stage = c.take(t.reg.stage);
    t.recs = c.take(t.reg.recs);
    compact_arrays(t, c, nchunks, 0);
    return t;
}

// ---- decompression: the scanned offsets (k + 1 u64, used when the caller passes none), then
//   frames: maxbpf block descriptors per frame (32 bytes each) | block statuses | frame statuses
//   zstd, snappy: the temp of the split decoder (decode_hip.hip carves it), where there is one
//   ragged: a block descriptor per chunk
// need_scan: the smallest temp that holds the scanned offsets.  need_split: the smallest temp with which the split
// decoder runs (0: this codec and chunk size have none); a smaller temp decodes every chunk whole.
struct DecodeTemp { size_t scan, desc, bstat, fstat, split, need_scan, need_split, total; };

// decode side of a framed layout: maxbpf descriptor slots per frame (blocks of 64 KiB / 32 KiB at the least)
static inline uint32_t frame_maxbpf(int codec, size_t F) {
    const size_t bmin = codec == LZH_CODEC_LZ4F ? 65536 : 32768;
    return (uint32_t)std::max<size_t>(1, (F + bmin - 1) / bmin);
}

static inline DecodeTemp decode_temp(int codec, size_t n, size_t chunk) {
    DecodeTemp t = {};
    TempCursor c;
    const size_t k = lzh_num_chunks(n, chunk);
    t.scan = c.take((k + 1) * sizeof(uint64_t));
    t.need_scan = c.at + kGap;
    if (codec == LZH_CODEC_LZ4F || codec == LZH_CODEC_NVLZ4) {
        const size_t nd = k * frame_maxbpf(codec, chunk);
        t.desc = c.take(nd * 32);
        t.bstat = c.take(nd * 4);
        t.fstat = c.take(k * 4, kGap);
    } else if (codec == LZH_CODEC_ZSTD || codec == LZH_CODEC_SNAPPY) {
        const size_t bytes = codec == LZH_CODEC_ZSTD ? lzh_zstd_decode_temp(n, chunk) : lzh_snappy_split_temp(n, chunk);
        t.split = c.take_sized(bytes);
        // (the zstd call has always asked for the whole sizing answer, the snappy call for the split's own bytes)
        if (bytes) t.need_split = codec == LZH_CODEC_ZSTD ? c.at + kGap : c.at;
    }
    t.total = c.at + kGap;
    return t;
}

static inline DecodeTemp ragged_decode_temp(size_t nchunks) {
    DecodeTemp t = {};
    TempCursor c;
    t.scan = c.take((nchunks + 1) * sizeof(uint64_t), kGap);
    t.need_scan = c.at;   // (the ragged call asks for the whole of `total`)
    t.desc = c.take(nchunks * 32, kGap);
    t.total = c.at;
    return t;
}

// ragged LZ4 frames (3i): the scanned offsets where ragged_decode_temp puts them, then the uniform frame decoder's
// regions for nchunks frames of up to max_bytes: frame_maxbpf descriptor slots per frame | block statuses | frame statuses
static inline DecodeTemp lz4f_ragged_decode_temp(size_t nchunks, size_t max_bytes) {
    DecodeTemp t = {};
    TempCursor c;
    const size_t nd = nchunks * frame_maxbpf(LZH_CODEC_LZ4F, max_bytes);
    t.scan = c.take((nchunks + 1) * sizeof(uint64_t), kGap);
    t.need_scan = c.at;
    t.desc = c.take(nd * 32);
    t.bstat = c.take(nd * 4);
    t.fstat = c.take(nchunks * 4, kGap);
    t.total = c.at;
    return t;
}

// ---- ragged zstd decompression with the four-kernel split decoder: the scanned offsets where ragged_decode_temp
// puts them, then the uniform decoder's per-frame layout for nchunks frames of max_bytes (decode_hip.hip zsplit):
//   nchunks frame areas of `stride` (blocks, tables, sequence records) | the sequence waves' dummy words, right
//   after them: the kernels address both from `frames` | frame states (i32) | frame fields | the Huffman jobs'
//   counter | the Huffman jobs
// No plan list: every launch is on the caller's stream.  ok = false (total 0): max_bytes below lzh_zstd_split_min
// or above 16 MiB, no split decoder.
struct ZstdRaggedSplitTemp {
    bool ok;
    size_t stride, scan, frames, dummy, state, fields, njobs, jobs, total;
    size_t frames_bytes, dummy_bytes, state_bytes, fields_bytes, jobs_bytes;
};
static inline ZstdRaggedSplitTemp zstd_ragged_split_temp(size_t nchunks, size_t max_bytes) {
    ZstdRaggedSplitTemp t = {};
    t.ok = max_bytes >= lzh_zstd_split_min && max_bytes <= kLz4SplitMax;
    if (!t.ok) return t;
    const LzhZstdSplitSizes z = lzh_zstd_split_sizes(max_bytes, nchunks);
    TempCursor c;
    t.stride = z.stride;
    t.scan = c.take((nchunks + 1) * sizeof(uint64_t), kGap);
    t.frames = c.take(t.frames_bytes = nchunks * z.stride);   // (a multiple of 256: the dummy words follow at once)
    t.dummy = c.take(t.dummy_bytes = z.dummy);
    t.state = c.take(t.state_bytes = nchunks * 4);
    t.fields = c.take(t.fields_bytes = nchunks * z.frame_fields);
    t.njobs = c.take(4);
    t.jobs = c.take(t.jobs_bytes = nchunks * z.frame_jobs, kGap);
    t.total = c.at;   // (above ragged_decode_temp's: a frame area alone is over 17 KiB)
    return t;
}

// ---- the same with the compact layout (zstd_split_slots.h; 3g's decode call and the debug calls of api.cpp): every
// frame's area laid out for the frame's own size and placed by a scan, the job list sized for the frames' own block
// slots.  The regions of zstd_ragged_split_temp
// in its order -- the area region and the job list sized by lzh_zstd_split_compact_regions for the promised total,
// the dummy words a region of their own -- then the placement's four arrays, as compact_arrays lays them out:
//   scanned offsets | area region | dummy words | frame states | frame fields | the Huffman jobs' counter | jobs
//   | area sizes | job counts (u32 each) | area offsets | job offsets (nchunks + 1 u64 each)
// The spare 256 bytes are those of zstd_ragged_split_temp (after the offsets and after the jobs) and the arrays
// follow without one, so the total never passes that layout's by more than the four arrays.  ok = false (total 0)
// exactly where zstd_ragged_split_temp's is.
struct ZstdRaggedSplitCompactTemp {
    bool ok;
    LzhZsplitRegions reg;
    size_t scan, areas, dummy, state, fields, njobs, jobs, area_sz, job_cnt, area_off, job_off, total;
    size_t dummy_bytes, state_bytes, fields_bytes, jobs_bytes;
};
static inline ZstdRaggedSplitCompactTemp zstd_ragged_split_compact_temp(size_t total_out, size_t max_bytes,
                                                                        size_t nchunks) {
    ZstdRaggedSplitCompactTemp t = {};
    t.ok = max_bytes >= lzh_zstd_split_min && max_bytes <= kLz4SplitMax;
    if (!t.ok) return t;
    const LzhZstdSplitSizes z = lzh_zstd_split_sizes(max_bytes, nchunks);
    const size_t job_bytes = lzh_zstd_split_sizes(0, 0).frame_jobs;   // (an empty frame has one block slot: one job)
    t.reg = lzh_zstd_split_compact_regions(total_out, max_bytes, nchunks);
    TempCursor c;
    t.scan = c.take((nchunks + 1) * sizeof(uint64_t), kGap);
    t.areas = c.take(t.reg.areas);
    t.dummy = c.take(t.dummy_bytes = z.dummy);
    t.state = c.take(t.state_bytes = nchunks * 4);
    t.fields = c.take(t.fields_bytes = nchunks * z.frame_fields);
    t.njobs = c.take(4);
    t.jobs = c.take(t.jobs_bytes = t.reg.jobs * job_bytes, kGap);
    t.area_sz = c.take(nchunks * 4);
    t.job_cnt = c.take(nchunks * 4);
    t.area_off = c.take((nchunks + 1) * 8);
    t.job_off = c.take((nchunks + 1) * 8);
    t.total = c.at;
    return t;
}
