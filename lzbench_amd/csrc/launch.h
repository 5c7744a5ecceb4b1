// lzbench_amd/csrc/launch.h -- host-side launchers exported by each kernel translation unit
// (internal to liblzbench_hip.so; the public C-ABI is include/lzbench_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// What every uniform compress launcher below is handed (include/lzbench_hip.h 3; api.cpp's uniform_call forms them
// once per call, the layouts of temp_layout.h hand out the slots).  The input: nchunks chunks, chunk i = the bytes from
// i * chunk_size of `in` (n_total bytes, in_readable may be read).  Framed layouts (LZ4 frame, nvcomp container): the
// chunks are the blocks -- block i is block i mod bpf of frame i / bpf, nframes frames of frame_size bytes cut into
// blocks of chunk_size.  bpf <= 1: plain chunks (frame_size unused, nframes = nchunks).
struct LzhInput {
    const uint8_t* in;
    uint64_t n_total, in_readable, chunk_size;
    uint32_t nchunks;
    uint64_t frame_size;
    uint32_t bpf, nframes;
};
// Uniform slots, each sized for the largest chunk (ragged: max_bytes), slot i for chunk i: staging slots of `stride`
// bytes; at recs, rec_stride apart, the LZ4 / snappy record slots or the zstd kernels' per-frame scratch areas (null /
// 0: the call has none); hdr: the per-chunk record counts (null where there are no records).
struct LzhSlots {
    uint8_t* stage;
    uint64_t stride;
    uint8_t* recs;
    uint64_t rec_stride;
    uint32_t* hdr;
};
// The slots of a framed layout: the blocks' slots (linked frames: the per-frame table snapshots, 16 KiB each, at
// blocks.recs), the block sizes and the block offsets inside their frame.
struct LzhFrameSlots {
    LzhSlots blocks;
    uint32_t *bcs, *rel;
};

hipError_t lzh_launch_lz4_compress_v2(const LzhInput& I, int acc, const LzhSlots& S, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_snappy_compress_v2(const LzhInput& I, const LzhSlots& S, uint32_t* csizes, hipStream_t s);
// desc: 32-byte block descriptors (frame_hip.hip) instead of chunk geometry + offsets / csizes
hipError_t lzh_launch_decompress(int codec, const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                 const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size, uint8_t* out,
                                 int32_t* status, uint32_t nchunks, hipStream_t s, const void* desc = nullptr);
hipError_t lzh_launch_zstd_decompress(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                      const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size, uint8_t* out,
                                      int32_t* status, uint32_t nchunks, uint8_t* zt, hipStream_t s);
size_t lzh_zstd_decode_temp(uint64_t n, uint64_t chunk_size);
// side stream k (0 or 1; highest priority, created once) of the caller's stream s and its fork / join events
// (decode_hip.hip): work forked to it after a record of `fork` on s joins back through `join`.  False (launch
// on s) when s belongs to another device than the current one.
bool lzh_side_stream(hipStream_t s, hipStream_t& ss, hipEvent_t& fork, hipEvent_t& join, int k = 0);
// snappy chunks of more than one 64 KiB fragment: split scan, fragments in parallel, serial fallback
size_t lzh_snappy_split_temp(uint64_t n, uint64_t chunk_size);
hipError_t lzh_launch_snappy_split_decompress(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                              const uint32_t* csizes, uint64_t n_total, uint64_t chunk_size, uint8_t* out,
                                              int32_t* status, uint32_t nchunks, uint8_t* temp, hipStream_t s);
// smallest chunk the zstd split decoder takes (below it: the one-wave decoder, no temp)
constexpr uint64_t lzh_zstd_split_min = 16384;
hipError_t lzh_launch_scan(const uint32_t* csizes, uint64_t nchunks, uint64_t* offsets, uint64_t* total, hipStream_t s);
hipError_t lzh_launch_pack(const LzhInput& I, const LzhSlots& S, const uint32_t* csizes, const uint64_t* offsets,
                           uint8_t* packed, uint64_t packed_cap, hipStream_t s);
hipError_t lzh_launch_memcpy(const void* src, void* dst, uint64_t n, hipStream_t s);
// scratch areas at S.recs, lzh_zstd_scratch_stride(chunk_size, level) apart (S.rec_stride is the layout's bound on it)
hipError_t lzh_launch_zstd_compress(const LzhInput& I, int level, const LzhSlots& S, uint32_t* csizes, hipStream_t s);
size_t lzh_zstd_scratch_stride(size_t chunk_size, int level);
int lzh_zstd_level_ok(int level, size_t chunk_size);
// dynamic LDS of the zstd match kernels for frames of up to chunk_size bytes (0: the hash table lives in scratch)
uint32_t lzh_zstd_lds_table(int level, uint64_t chunk_size);
// zstd level 3, the double-fast strategy (zstdc_dfast_hip.hip; LZH_CODEC_ZSTD_DFAST): scratch areas at S.recs,
// lzh_zstd_dfast_scratch_stride(chunk_size) apart -- the fast levels' areas below the table, then the long and the
// short table, each the largest of any chunk size up to chunk_size.  One match / entropy pair per block index, every
// launch on s: no side stream, so a captured call has no parallel branches.
hipError_t lzh_launch_zstd_dfast_compress(const LzhInput& I, int level, const LzhSlots& S, uint32_t* csizes,
                                          hipStream_t s);
size_t lzh_zstd_dfast_scratch_stride(size_t chunk_size);
// What every ragged compress launcher below is handed (include/lzbench_hip.h 3b .. 3h; api.cpp's ragged_compress
// forms them, the layouts of temp_layout.h hand out the slots).
// The batch: chunk i = bytes[i] bytes at ptrs[i] (device arrays of nchunks).  A chunk larger than max_bytes is not
// processed: csizes[i] = 0, no kernel touches its slots.
struct LzhBatch {
    const void* const* ptrs;
    const uint64_t* bytes;
    uint64_t max_bytes;
    uint32_t nchunks;
};

// ragged zstd batches (zstd_ragged_hip.hip, zstd_ragged_decode_hip.hip, zstd_ragged_split_hip.hip;
// include/lzbench_hip.h 3c): staging slots and scratch areas as chunk_temp(LZH_CODEC_ZSTD, nchunks, max_bytes) lays
// them out (rec_stride at least lzh_zstd_scratch_stride(max_bytes, level)).  Every launch on s.  On the decode side a
// chunk larger than max_bytes gets status[i] = -1.
hipError_t lzh_launch_zstd_ragged(const LzhBatch& B, int level, const LzhSlots& S, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_zstd_decompress_ragged(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                             const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                                             uint64_t max_bytes, int32_t* status, uint32_t nchunks, hipStream_t s);
// the same through the four-kernel split decoder (zstd_ragged_split_hip.hip); split: its temp regions
// (ZstdRaggedSplitTemp, temp_layout.h), laid out for nchunks frames of up to max_bytes.  Frames it leaves decode in
// the one-wave kernel; with lzh_debug_zstd_legacy(1) the call is the one above.
struct LzhZstdSplitTemp {
    uint8_t* frames;     // nchunks per-frame areas, the sequence waves' dummy words right after them
    int32_t* state;      // nchunks frame states (kGo 0, kLegacy 1, kDone 2)
    void* zfr;           // nchunks frame fields
    uint32_t* njobs;     // the Huffman jobs' counter
    void* jobs;          // nchunks x (blocks per frame) Huffman jobs
};
hipError_t lzh_launch_zstd_decompress_ragged_split(const uint8_t* packed, uint64_t packed_readable,
                                                   const uint64_t* offsets, const uint32_t* csizes,
                                                   void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                                                   int32_t* status, uint32_t nchunks, const LzhZstdSplitTemp& split,
                                                   hipStream_t s);
// the compact temp layout of the split decoder (zstd_split_slots.h derives it; host arithmetic for api.cpp's sizing
// and debug calls): the two regions that hold every batch of at most nchunks frames of at most max_bytes that
// sums to at most total bytes, and the {area bytes, Huffman job slots} of a frame of n bytes
struct LzhZsplitRegions { uint64_t areas, jobs; };   // (bytes; Huffman jobs)
LzhZsplitRegions lzh_zstd_split_compact_regions(uint64_t total, uint64_t max_bytes, uint64_t nchunks);
LzhZsplitRegions lzh_zstd_split_compact_slot(uint64_t n);
// the split decoder through that layout (zstd_ragged_split_compact_hip.hip; include/lzbench_hip.h 3g).  T: the regions of
// ZstdRaggedSplitCompactTemp (temp_layout.h); `slots` is the compress side's layout struct (below) carrying the
// placement -- stage_sz / stage_off / stage_cap: the area sizes, their scan, the area region's bytes; rec_sz / rec_off /
// rec_cap: the job counts, their scan, the job list's slots.  The call fills the four arrays, sets the frame states
// (a chunk over max_bytes: kDone, status -1; a frame that ends outside a region: kLegacy) and runs the split kernels
// and the one-wave kernel, every launch on s; with lzh_debug_zstd_legacy(1) it is lzh_launch_zstd_decompress_ragged.
struct LzhCompactLayout;
struct LzhZstdSplitCompactTemp;
hipError_t lzh_launch_zstd_decompress_ragged_sel(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                                 const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                                                 uint64_t max_bytes, int32_t* status, uint32_t nchunks,
                                                 const int32_t* zsel, hipStream_t s);
hipError_t lzh_launch_zstd_decompress_ragged_split_compact(const uint8_t* packed, uint64_t packed_readable,
                                                           const uint64_t* offsets, const uint32_t* csizes,
                                                           void* const* out_ptrs, const uint64_t* out_bytes,
                                                           uint64_t max_bytes, int32_t* status, uint32_t nchunks,
                                                           const LzhZstdSplitCompactTemp& T, hipStream_t s);
// decode_hip.hip, for the ragged launcher and its layout: the sizes of the split decoder's temp for nchunks frames of
// up to `chunk` bytes (a frame's area, the dummy words, a frame's fields, a frame's Huffman jobs); the test hooks
// lzh_debug_zstd_legacy / _hufpar and the Huffman sections a wave (4 or 8: the hook, else by nchunks and the device's
// CUs); the sequence kernel, which knows no output geometry, over every frame on s
struct LzhZstdSplitSizes { size_t stride, dummy, frame_fields, frame_jobs; };
LzhZstdSplitSizes lzh_zstd_split_sizes(uint64_t chunk, uint64_t nchunks);
struct LzhZstdHooks { int legacy, hufpar, huf_sections; };
LzhZstdHooks lzh_zstd_hooks(uint32_t nchunks);
hipError_t lzh_launch_zstd_seq(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                               uint64_t slot_bytes, uint32_t nchunks, int32_t* status, uint8_t* zt, const int32_t* zst,
                               void* zfr, hipStream_t s);
// linked LZ4 frames, one wave per frame (I: the blocks of a framed layout; the block sizes go to F.bcs)
hipError_t lzh_launch_lz4f_linked(const LzhInput& I, int acc, const LzhFrameSlots& F, hipStream_t s);
// parse kernel, emit kernel: stage_mask bit 0 = parse, bit 1 = emit (framed layouts: csizes = the block sizes)
hipError_t lzh_launch_lz4_split(const LzhInput& I, int acc, const LzhSlots& S, uint32_t* csizes, int stage_mask,
                                hipStream_t s);
size_t lzh_lz4_rec_stride(uint64_t chunk_size);
hipError_t lzh_launch_snappy_split(const LzhInput& I, const LzhSlots& S, uint32_t* csizes, int stage_mask, hipStream_t s);
size_t lzh_snappy_rec_stride(uint64_t chunk_size);
uint32_t lzh_snappy_frags(uint64_t chunk_size);
// the emit kernel of a snappy launcher by waves per block: k1 for chunks of one fragment, else the kernel with
// kW >= min(frags, 8) waves (the block has exactly that many); args: the kernels' common arguments
template <class K1, class K2, class K4, class K8, class... Args>
void lzh_launch_snappy_emit(K1 k1, K2 k2, K4 k4, K8 k8, uint32_t frags, uint32_t nchunks, hipStream_t s, Args... args) {
    const uint32_t W = frags < 8 ? frags : 8;
    if (W <= 1) hipLaunchKernelGGL(k1, dim3(nchunks), dim3(64), 0, s, args...);
    else if (W == 2) hipLaunchKernelGGL(k2, dim3(nchunks), dim3(128), 0, s, args...);
    else if (W <= 4) hipLaunchKernelGGL(k4, dim3(nchunks), dim3(64 * W), 0, s, args...);
    else hipLaunchKernelGGL(k8, dim3(nchunks), dim3(64 * W), 0, s, args...);
}

// ragged batches (ragged_hip.hip, pack_hip.hip): the slots as chunk_temp(codec, nchunks, max_bytes) of temp_layout.h
// lays them out; the pack launcher reads the staging slots alone
hipError_t lzh_launch_lz4_ragged(const LzhBatch& B, int acc, const LzhSlots& S, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_snappy_ragged(const LzhBatch& B, const LzhSlots& S, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_pack_ragged(const LzhBatch& B, const LzhSlots& S, const uint32_t* csizes, const uint64_t* offsets,
                                  uint8_t* packed, uint64_t packed_cap, hipStream_t s);
// fragments per chunk of a ragged snappy batch (at least 1: the launch grid of a batch of empty chunks)
uint32_t lzh_snappy_ragged_frags(uint64_t max_bytes);
// block descriptors (32 bytes each, for lzh_launch_decompress) of a ragged batch: absolute output addresses;
// an out_bytes[i] above max_bytes gives a skipped descriptor and status[i] = -1
hipError_t lzh_launch_ragged_desc(const uint64_t* offsets, const uint32_t* csizes, void* const* out_ptrs,
                                  const uint64_t* out_bytes, uint64_t max_bytes, void* desc, int32_t* status,
                                  uint32_t nchunks, hipStream_t s);

// LZ4 ragged batches with a shared dictionary (lz4_dict_hip.hip; include/lzbench_hip.h 3d): dict_bytes in 8 .. 65536,
// 16 readable bytes after the dictionary; tab: 4096 u32 of temp for LZ4_loadDict's table, built by the call; staging
// slots alone, no records.  Every launch on s.  On the decode side a chunk larger than max_bytes gets status[i] = -1.
hipError_t lzh_launch_lz4_dict(const uint8_t* dict, uint32_t dict_bytes, uint32_t* tab, const LzhBatch& B, int acc,
                               const LzhSlots& S, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_lz4_dict_decompress(const uint8_t* dict, uint32_t dict_bytes, const uint8_t* packed,
                                          uint64_t packed_readable, const uint64_t* offsets, const uint32_t* csizes,
                                          void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                                          int32_t* status, uint32_t nchunks, hipStream_t s);

// the compact layout of a ragged compression (ragged_compact_hip.hip, ragged_slots.h): chunk i's staging slot is
// stage_sz[i] bytes at stage_off[i] of a staging region of stage_cap bytes, its record slot rec_sz[i] bytes at
// rec_off[i] of a record region of rec_cap bytes (device arrays: nchunks u32, nchunks + 1 u64).
// lzh_launch_compact_slots fills the four arrays (the slot-size kernel, then lzh_launch_compact_scans: the offset
// arrays from the size arrays, lzh_launch_scan twice); the other launchers are the ragged ones above with the slots
// looked up there.  A chunk larger than max_bytes, or one with a slot that ends past its region, gets csizes[i] = 0.
// (the arrays are written by lzh_launch_compact_slots alone; every other kernel takes the struct as const)
struct LzhCompactLayout {
    uint32_t* stage_sz;
    uint32_t* rec_sz;
    uint64_t* stage_off;
    uint64_t* rec_off;
    uint64_t stage_cap, rec_cap;
};
struct LzhZstdSplitCompactTemp {
    uint8_t* areas;      // the area region
    uint8_t* dummy;      // the sequence waves' dummy words
    int32_t* state;      // nchunks frame states
    void* zfr;           // nchunks frame fields
    uint32_t* njobs;     // the Huffman jobs' counter
    void* jobs;          // slots.rec_cap Huffman jobs
    LzhCompactLayout slots;
};
// Compact slots, what LzhSlots is to the uniform ones: the staging region, the record region (zstd: the scratch
// region), the per-chunk record counts (null where there are no records) and the placement.
struct LzhCompactSlots {
    uint8_t* stage;
    uint8_t* recs;
    uint32_t* hdr;
    LzhCompactLayout L;
};
hipError_t lzh_launch_compact_scans(const LzhCompactLayout& L, uint32_t nchunks, hipStream_t s);
hipError_t lzh_launch_compact_slots(int codec, const LzhBatch& B, const LzhCompactLayout& L, hipStream_t s);
hipError_t lzh_launch_lz4_compact(const LzhBatch& B, int acc, const LzhCompactSlots& S, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_snappy_compact(const LzhBatch& B, const LzhCompactSlots& S, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_pack_compact(const LzhBatch& B, const LzhCompactSlots& S, const uint32_t* csizes,
                                   const uint64_t* offsets, uint8_t* packed, uint64_t packed_cap, hipStream_t s);

// the compact layout of a ragged zstd compression (zstd_ragged_compact_hip.hip, zstd_ragged_slots.h): the layout
// struct above with the record fields carrying the scratch slots -- chunk i's scratch slot is rec_sz[i] bytes at
// rec_off[i] of a scratch region of rec_cap bytes.  lzh_launch_zstd_compact fills the four arrays (the zstd
// slot-size kernel, then lzh_launch_compact_scans) and runs the match / entropy pair per block index, every launch on
// s; lzh_launch_pack_compact above packs.  A chunk larger than max_bytes, or one with a slot that ends past its
// region, gets csizes[i] = 0.  The two host functions are the slot arithmetic for api.cpp (sizing, host mirror):
// the two regions, and the two slots of a chunk of n bytes, each as {staging bytes, scratch bytes}.
struct LzhCompactRegions;   // ragged_slots.h
LzhCompactRegions lzh_zstd_compact_regions(int level, uint64_t total, uint64_t max_bytes, uint64_t nchunks);
LzhCompactRegions lzh_zstd_compact_slot(int level, uint64_t n);
hipError_t lzh_launch_zstd_compact(const LzhBatch& B, int level, const LzhCompactSlots& S, uint32_t* csizes,
                                   hipStream_t s);

// ragged zstd level-3 batches (zstd_dfast_ragged_hip.hip, zstd_dfast_slots.h; include/lzbench_hip.h 3e): the
// launchers of the two layouts above for the double-fast strategy.  lzh_launch_zstd_dfast_ragged: scratch areas
// rec_stride apart (at least lzh_zstd_dfast_scratch_stride(max(max_bytes, 1))).  lzh_launch_zstd_dfast_compact: the compact layout struct with the record fields carrying the scratch
// slots; it fills the four arrays (the level-3 slot-size kernel, then lzh_launch_compact_scans).  Both run one match /
// entropy pair per block index, ceil(max(max_bytes, 1) / block size) of them, every launch on s; level must be 3.
// A chunk larger than max_bytes, or (compact) one with a slot that ends past its region, gets csizes[i] = 0.  The two
// host functions are the slot arithmetic as {staging bytes, scratch bytes}: the two regions, a chunk's two slots.
hipError_t lzh_launch_zstd_dfast_ragged(const LzhBatch& B, int level, const LzhSlots& S, uint32_t* csizes,
                                        hipStream_t s);
hipError_t lzh_launch_zstd_dfast_compact(const LzhBatch& B, int level, const LzhCompactSlots& S, uint32_t* csizes,
                                         hipStream_t s);
LzhCompactRegions lzh_zstd_dfast_compact_regions(uint64_t total, uint64_t max_bytes, uint64_t nchunks);
LzhCompactRegions lzh_zstd_dfast_compact_slot(uint64_t n);

// ragged zstd batches with a shared dictionary (zstd_dict_hip.hip, zstd_dict_parse.h; include/lzbench_hip.h 3f):
// dict_bytes in 8 .. 131072 and max_bytes <= 131072, 16 readable bytes after the dictionary; levels 1, -1 .. -5.
// lzh_zstd_dict_scratch_stride: a chunk's scratch area (the areas of the zstd kernels' Layout for a block of max_bytes,
// then the frame's own copy of its class's table); lzh_zstd_dict_tables_bytes: the table region (one filled table per
// (hashLog, minMatch) class a batch can take, a constant bound).  The compress launcher fills the class tables once,
// then runs the match kernel and the entropy stage of lzh_launch_zstd_entropy_ragged (zstd_ragged_hip.hip), every
// launch on s (seq_off .. tmp_off: the four areas of a frame's scratch that the entropy stage reads).  On the decode
// side a chunk larger than max_bytes gets status[i] = -1.
size_t lzh_zstd_dict_scratch_stride(size_t dict_bytes, size_t max_bytes);
size_t lzh_zstd_dict_tables_bytes(void);
hipError_t lzh_launch_zstd_dict(const uint8_t* dict, uint32_t dict_bytes, uint8_t* tables, const LzhBatch& B, int level,
                                const LzhSlots& S, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_zstd_entropy_ragged(const LzhBatch& B, int level, const LzhSlots& S, uint32_t* csizes,
                                          uint64_t seq_off, uint64_t lit_off, uint64_t att_off, uint64_t tmp_off,
                                          hipStream_t s);
hipError_t lzh_launch_zstd_dict_decompress(const uint8_t* dict, uint32_t dict_bytes, const uint8_t* packed,
                                           uint64_t packed_readable, const uint64_t* offsets, const uint32_t* csizes,
                                           void* const* out_ptrs, const uint64_t* out_bytes, uint64_t max_bytes,
                                           int32_t* status, uint32_t nchunks, hipStream_t s);
// host arithmetic for the debug calls: ZSTD_getParams(level, n, dict_bytes) as {windowLog, hashLog, minMatch,
// targetLength, block size}, and the host walk of one chunk ((ll, ml, offBase) triples; the count, -1: arguments)
int lzh_zstd_dict_params(int level, uint64_t n, uint64_t dict_bytes, uint32_t* out);
long lzh_zstd_dict_host_parse(int level, const uint8_t* dict, uint64_t dict_bytes, const uint8_t* src, uint64_t n,
                              uint32_t* seqs, uint64_t cap);

// ragged zstd level-3 batches with a shared dictionary (zstd_dfast_dict_hip.hip, zstd_dfast_dict_parse.h;
// include/lzbench_hip.h 3h): 3f's limits, level 3 alone.  lzh_zstd_dfast_dict_scratch_stride: a chunk's scratch area
// (the areas of the zstd kernels' Layout for a block of max_bytes, then the frame's private pair of tables, the largest
// any frame of the batch can take); lzh_zstd_dfast_dict_tables_bytes: the table region (one filled pair per (hashLog,
// chainLog, minMatch) class, a constant bound).  The launcher fills the class tables once, then runs the match kernel
// and the level-3 entropy stage of lzh_launch_zstd_dfast_entropy_ragged (zstd_dfast_ragged_hip.hip: block 0 of
// lzh_zstd_dfast_entropy_ragged_kernel alone), every launch on s.
size_t lzh_zstd_dfast_dict_scratch_stride(size_t dict_bytes, size_t max_bytes);
size_t lzh_zstd_dfast_dict_tables_bytes(void);
hipError_t lzh_launch_zstd_dfast_dict(const uint8_t* dict, uint32_t dict_bytes, uint8_t* tables, const LzhBatch& B,
                                      int level, const LzhSlots& S, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_zstd_dfast_entropy_ragged(const LzhBatch& B, int level, const LzhSlots& S, uint32_t* csizes,
                                                uint64_t seq_off, uint64_t lit_off, uint64_t att_off, uint64_t tmp_off,
                                                hipStream_t s);
// host arithmetic for the debug calls: {windowLog, hashLog, chainLog, minMatch, block size} of ZSTD_getParams(3, n,
// dict_bytes), and the host walk of one chunk ((ll, ml, offBase) triples and, where events is not null, the counters
// of zfd::Event added to it; the count, -1: arguments)
int lzh_zstd_dfast_dict_params(int level, uint64_t n, uint64_t dict_bytes, uint32_t* out);
long lzh_zstd_dfast_dict_host_parse(int level, const uint8_t* dict, uint64_t dict_bytes, const uint8_t* src, uint64_t n,
                                    uint32_t* seqs, uint64_t cap, uint64_t* events);

// framed LZ4 layouts (frame_hip.hip); codec 4 = LZ4 frame, 5 = nvcomp LZ4 container
// (I: the blocks of the framed layout; params: the call's level; csizes: the frame sizes)
hipError_t lzh_launch_frame_sizes(const LzhInput& I, int codec, int params, const uint32_t* bcs, uint32_t* rel,
                                  uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_frame_pack(const LzhInput& I, int codec, int params, const LzhFrameSlots& F, const uint32_t* csizes,
                                 const uint64_t* offsets, uint8_t* packed, hipStream_t s);
hipError_t lzh_launch_frame_parse(int codec, const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                  const uint32_t* csizes, uint64_t n_total, uint64_t fs, uint32_t maxbpf, void* desc,
                                  int32_t* fstat, uint32_t nframes, hipStream_t s);
hipError_t lzh_launch_frame_finish(int codec, const uint8_t* packed, const uint64_t* offsets, const uint32_t* csizes,
                                   uint64_t n_total, uint64_t fs, uint32_t maxbpf, const void* desc,
                                   const int32_t* bstat, const int32_t* fstat, const uint8_t* out, int32_t* status,
                                   uint32_t nframes, hipStream_t s);

// ragged LZ4 frames (lz4f_ragged_hip.hip; include/lzbench_hip.h 3i): a frame per chunk of the batch, the frames'
// blocks laid out for the largest chunk -- blocks of bs = min(the level's block size, max_bytes), bpf = ceil(max_bytes
// / bs) block slots per frame, frame i's at i * bpf.  F: the slots of nchunks * bpf blocks as frame_temp lays them
// out; bptrs / bbytes: the derived block batch (nchunks * bpf entries each), written by lzh_launch_lz4f_ragged and
// handed to lzh_launch_lz4_ragged as a batch with max_bytes = bs; params: the call's level.
struct LzhRaggedFrame {
    LzhFrameSlots F;
    const void** bptrs;
    uint64_t* bbytes;
    uint64_t bs;
    uint32_t bpf;
    int params;
};
// block table -> the ragged LZ4 parse and emit kernels over the blocks (sizes to F.bcs) -> the frame sizes (csizes;
// 0 for a chunk larger than max_bytes) and the block offsets (F.rel); then, after the scan, the pack: a frame whose
// packed range would pass packed_cap is not written.  Every launch on s.
hipError_t lzh_launch_lz4f_ragged(const LzhBatch& B, int acc, const LzhRaggedFrame& R, uint32_t* csizes, hipStream_t s);
hipError_t lzh_launch_lz4f_pack_ragged(const LzhBatch& B, const LzhRaggedFrame& R, const uint32_t* csizes,
                                       const uint64_t* offsets, uint8_t* packed, uint64_t packed_cap, hipStream_t s);
// frame i decodes to out_bytes[i] bytes at out_ptrs[i]: the ragged frame parse (maxbpf descriptor slots per frame at
// desc, frame statuses at fstat), lzh_launch_decompress over the nchunks * maxbpf descriptors with a null output base
// (block statuses at bstat), the ragged frame finish.  An out_bytes[i] above max_bytes gives status[i] = -1.
hipError_t lzh_launch_lz4f_decompress_ragged(const uint8_t* packed, uint64_t packed_readable, const uint64_t* offsets,
                                             const uint32_t* csizes, void* const* out_ptrs, const uint64_t* out_bytes,
                                             uint64_t max_bytes, int32_t* status, uint32_t nchunks, uint32_t maxbpf,
                                             void* desc, int32_t* bstat, int32_t* fstat, hipStream_t s);
