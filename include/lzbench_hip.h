/*
 * include/lzbench_hip.h -- C-ABI of liblzbench_hip.so, the MI355X (gfx950) drop-in for the
 * lzbench chunk-loop hot path (LZ4 block + snappy raw codecs, bit-exact with the reference
 * lz4 1.9.3 / snappy 1.1.8).  Plain pointers and sizes only.
 *
 * Three layers:
 *
 *  1. lzbench rows -- the exact compressor_desc_t function-pointer signatures of
 *     /root/reference/_lzbench/lzbench.h:113-115, so a maintainer adds rows to comp_desc[]
 *     (lzbench.h:140-219) next to the CUDA rows (lzbench.h:217-218) under BENCH_HAS_HIP:
 *       compress_func   int64_t (*)(char *in, size_t insize, char *out, size_t outsize,
 *                                   size_t level, size_t param2, char *workmem)
 *       init_func       char* (*)(size_t chunk_size, size_t level, size_t ngpus)
 *       deinit_func     void (*)(char *workmem)
 *     Replaces: lzbench_lz4_compress / lzbench_lz4fast_compress / lzbench_lz4_decompress
 *     (compressors.cpp:343-362), lzbench_snappy_compress / _decompress (compressors.cpp:1282-1292),
 *     lzbench_cuda_{init,deinit,memcpy,return_0} and lzbench_nvcomp_* (compressors.cpp:1813-2014).
 *     Error conventions are lzbench's (lzbench.cpp:284-288, :321): compress returns the
 *     compressed length, <= 0 on failure (driver then stores raw); decompress returns the
 *     decompressed length, <= 0 on error.
 *
 *  2. batched rows -- one call per chunk list instead of one per chunk (the per-chunk ABI
 *     serialises a GPU); replaces the two chunk loops
 *     lzbench_compress / lzbench_decompress (lzbench.cpp:266-298 / :301-329) including the
 *     raw-store rule (clen <= 0 || clen == part -> stored raw, compr_size = part) and the
 *     contiguous packing in chunk order.  Chunks are sharded over the GPUs given to init
 *     (param2 = ngpus): the chunk list is cut into ~128 MiB sub-batches of consecutive chunks,
 *     dealt round-robin to the devices (each pipelines copy-in / kernels / copy-out on its own
 *     streams), and one host-side gather copies every sub-batch's packed bytes to its chunk-order
 *     offset as soon as its sizes land -- so no device's copy-out waits for the devices before it
 *     to finish their whole share.  (One process per GPU under torchrun instead gives each rank
 *     one contiguous slab, lzbench_amd/shard.py)
 *
 *  3. device-resident API -- inputs already in HBM, asynchronous on a caller stream
 *     (the nvcomp batched API analogue, reference nvcomp/lz4.h:239-371).  The input is n
 *     bytes cut into ceil(n/chunk_size) chunks of chunk_size (last one ragged).
 *     Readable-size arguments give how many bytes past the start may be read (>= n + 16):
 *     kernels read whole dwords and rely on that slack.
 */
#ifndef LZBENCH_HIP_H
#define LZBENCH_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* LZH_CODEC_ZSTD: zstd 1.5.2 frames as lzbench's zstd rows write them, one frame per chunk
 * (ZSTD_getParams(level, chunk, 0) + content size, no dictionary, no checksum).  Compression:
 * the fast-strategy levels (zstd 1, 2 where fast, zstd_fast -1..-5), bit-exact with the reference;
 * other levels return LZH_EARG.  Decoding: any frame of that shape, also with the XXH64 content
 * checksum (verified); dictionary ids, a missing content size or windows over 2^27 report -2. */
/* LZH_CODEC_LZ4F: one LZ4 frame per chunk as LZ4F_compressFrame writes it (lz4/lz4frame.c:429-470)
 * with independent blocks, or linked blocks with LZH_LZ4F_LINKED (LZ4_compress_fast_continue in prefix
 * mode, lz4.c:1565-1628); level = LZH_LZ4F_PARAMS(blockSizeID 0|4..7, flags, acceleration).
 * Decoding: frames with independent or linked blocks, every block but the last full, no dictionary id;
 * other frames report -2.
 * LZH_CODEC_NVLZ4: one nvcomp LZ4 container per chunk (the format of the reference's nvcomp_lz4
 * row, nvcomp/LZ4Metadata.h), LZ4 blocks of 1 << (15 + level) bytes, level 0..5 (compressors.cpp:1863).
 * Both: lzh_compress_async / lzh_decompress_async and the rows below; not lzh_compress_kernel_only /
 * lzh_compress_finish_async. */
/* LZH_CODEC_ZSTD_DFAST: zstd 1.5.2 frames at the levels whose ZSTD_getParams row is ZSTD_dfast (double-fast) for
 * every chunk size: level 3, zstd's own default (clevels.h:25-111: dfast in all four source-size tables).  Same
 * frame shape as LZH_CODEC_ZSTD, bit-exact with the reference; every other level returns LZH_EARG (level 2 is fast
 * in two tables and dfast in one, level 4 greedy in two: neither is one code path for a batch).  LZH_CODEC_ZSTD
 * itself keeps refusing level 3.
 * With this codec: lzh_stage_stride and lzh_max_packed_bytes equal LZH_CODEC_ZSTD's; lzh_compress_temp_bytes sizes
 * the per-frame scratch with the two dfast tables (long 4 << hashLog + short 4 << chainLog bytes: 768 KiB a frame
 * for chunks over 256 KiB, 192 KiB at 16 KiB) and is never below LZH_CODEC_ZSTD's; lzh_compress_async takes chunk
 * sizes up to 16 MiB (larger: LZH_EARG) and checks in the uniform call's order (arguments, temp_bytes and
 * packed_cap: LZH_ESPACE, then level and chunk size: LZH_EARG), every launch on hip_stream (no side stream: a
 * captured call has no parallel branches); lzh_decompress_temp_bytes and lzh_decompress_async are LZH_CODEC_ZSTD's
 * (the frames also decode with LZH_CODEC_ZSTD).  lzh_compress_kernel_only, lzh_compress_kernel_stage,
 * lzh_compress_finish_async, the ragged calls (3b) return LZH_EARG for it and their temp sizing functions 0; the
 * ragged zstd calls (3c) keep refusing level 3, and the dictionary calls (3d) are LZ4's. */
enum { LZH_CODEC_LZ4 = 0, LZH_CODEC_SNAPPY = 1, LZH_CODEC_MEMCPY = 2, LZH_CODEC_ZSTD = 3, LZH_CODEC_LZ4F = 4,
       LZH_CODEC_NVLZ4 = 5, LZH_CODEC_ZSTD_DFAST = 6 };
#define LZH_LZ4F_BLOCK_CHECKSUM   0x10   /* LZ4F_blockChecksumEnabled */
#define LZH_LZ4F_CONTENT_CHECKSUM 0x20   /* LZ4F_contentChecksumEnabled */
#define LZH_LZ4F_CONTENT_SIZE     0x40   /* frameInfo.contentSize = chunk size */
#define LZH_LZ4F_LINKED           0x80   /* LZ4F_blockLinked (the LZ4F default; frames of one block stay independent) */
#define LZH_LZ4F_PARAMS(bsid, flags, acc) ((bsid) | (flags) | ((acc) << 8))
enum { LZH_OK = 0, LZH_EARG = -1, LZH_EHIP = -2, LZH_ESPACE = -3, LZH_ECORRUPT = -4 };

/* ---- 1. lzbench rows (per-chunk ABI) ------------------------------------------------ */
char*   lzbench_hip_lz4_init(size_t chunk_size, size_t level, size_t ngpus);
char*   lzbench_hip_snappy_init(size_t chunk_size, size_t level, size_t ngpus);
char*   lzbench_hip_memcpy_init(size_t chunk_size, size_t level, size_t ngpus);
char*   lzbench_hip_zstd_init(size_t chunk_size, size_t level, size_t ngpus);
char*   lzbench_hip_zstd_dfast_init(size_t chunk_size, size_t level, size_t ngpus);
char*   lzbench_hip_lz4frame_init(size_t chunk_size, size_t level, size_t ngpus);
char*   lzbench_hip_nvcomp_lz4_init(size_t chunk_size, size_t level, size_t ngpus);
void    lzbench_hip_deinit(char* workmem);
/* lz4: LZ4_compress_default semantics; lz4fast: level = acceleration (LZ4_compress_fast) */
int64_t lzbench_hip_lz4_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
int64_t lzbench_hip_lz4fast_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
int64_t lzbench_hip_lz4_decompress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
int64_t lzbench_hip_snappy_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
int64_t lzbench_hip_snappy_decompress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
/* zstd: lzbench_zstd_compress / _decompress semantics (compressors.cpp:1745-1778); level as the
 * zstd / zstd_fast rows pass it (size_t of a possibly negative int) */
int64_t lzbench_hip_zstd_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
int64_t lzbench_hip_zstd_decompress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
/* zstd level 3 (LZH_CODEC_ZSTD_DFAST, workmem from lzbench_hip_zstd_dfast_init): level must be 3.  Decompression is
 * lzbench_hip_zstd_decompress, which takes a workmem of either zstd init */
int64_t lzbench_hip_zstd_dfast_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
/* LZ4 frame per chunk: level = LZH_LZ4F_PARAMS(...): 4..7 = blockSizeID 64 KiB .. 4 MiB without flags,
 * e.g. 0x74 = 64 KiB blocks + block / content checksums + content size */
int64_t lzbench_hip_lz4frame_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
int64_t lzbench_hip_lz4frame_decompress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
/* nvcomp LZ4 container per chunk: replaces lzbench_nvcomp_compress / _decompress (compressors.cpp:1916-2014),
 * level 0..5 = chunks of 32 KiB << level */
int64_t lzbench_hip_nvcomp_lz4_compress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
int64_t lzbench_hip_nvcomp_lz4_decompress(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);
/* hipMemcpy plumbing row: host -> HBM -> host round trip of the chunk */
int64_t lzbench_hip_memcpy(char* in, size_t insize, char* out, size_t outsize, size_t level, size_t p2, char* workmem);

/* ---- 2. batched rows ----------------------------------------------------------------- */
/* Compress nchunks consecutive chunks of in (sizes chunk_sizes[]) into out (capacity
 * outcap), filling compr_sizes[]; applies the raw-store rule. Returns total packed bytes,
 * <= 0 on failure.  The codec and level come from the init call that made workmem. */
int64_t lzbench_hip_compress_batch(const char* in, const size_t* chunk_sizes, int nchunks, char* out,
                                   size_t outcap, size_t* compr_sizes, size_t level, size_t p2, char* workmem);
/* Inverse: out receives sum(chunk_sizes) bytes. Returns that total, <= 0 on error. */
int64_t lzbench_hip_decompress_batch(const char* in, const size_t* compr_sizes, const size_t* chunk_sizes,
                                     int nchunks, char* out, size_t outcap, size_t level, size_t p2, char* workmem);

/* ---- 3. device-resident API ---------------------------------------------------------- */
/* bytes of the per-chunk staging slot (>= worst-case compressed chunk, 256-aligned) */
size_t lzh_stage_stride(int codec, size_t chunk_size);
/* upper bound of the packed output for n bytes */
size_t lzh_max_packed_bytes(int codec, size_t n, size_t chunk_size);
size_t lzh_compress_temp_bytes(int codec, size_t n, size_t chunk_size);
size_t lzh_decompress_temp_bytes(int codec, size_t n, size_t chunk_size);
size_t lzh_num_chunks(size_t n, size_t chunk_size);
/* 1 when the GPU codec compresses at `level` for chunks of up to chunk_size bytes, else 0 (the
 * rows and lzh_compress_async then return LZH_EARG): zstd at the levels whose ZSTD_getParams row
 * is the fast strategy for every chunk size up to chunk_size (lzbench's zstd level 2 is double-fast
 * above 256 KiB: compressors.cpp:1752 via clevels.h); LZH_CODEC_ZSTD_DFAST at level 3 alone, for any chunk_size;
 * LZ4F / nvcomp at the parameters above. */
int lzh_level_supported(int codec, int level, size_t chunk_size);
/* The batched rows' sharding plan (api.cpp make_plan) and per-shard buffer sizes for n bytes in
 * chunks of chunk_size over ngpus shards, into out[0 .. nout): chunks, chunks per sub-batch,
 * sub-batches, shards, compress input / packed / temp bytes per sub-batch slot, then the sub-batch
 * slots of shard 0 .. shards-1.  Host arithmetic only (no device call).  Returns the count written. */
int lzh_debug_plan(size_t ngpus, size_t n, size_t chunk_size, int codec, uint64_t* out, int nout);
/* The batched rows' host gather order (api.cpp GatherOrder): sub-batches 0 .. nsb-1 complete in
 * `order` (a permutation) with packed sizes sizes[j]; placed[3i .. 3i+2] = (sub-batch, output offset,
 * index into `order` of the completion that made it placeable) for the i-th placement.  Host
 * arithmetic only.  Returns the number of placements (nsb). */
int lzh_debug_gather_order(size_t nsb, const uint64_t* order, const uint64_t* sizes, uint64_t* placed);

/* d_csizes: nchunks u32 (out); d_offsets: nchunks+1 u64 (out; [nchunks] = packed total).
 * level: lz4 acceleration (<=1 -> LZ4_compress_default); zstd level; ignored by snappy. */
int lzh_compress_async(int codec, int level, const void* d_in, size_t n, size_t in_readable, size_t chunk_size,
                       void* d_packed, size_t packed_cap, uint32_t* d_csizes, uint64_t* d_offsets,
                       void* d_temp, size_t temp_bytes, void* hip_stream);
/* d_offsets may be NULL (then derived from d_csizes into d_temp).  d_temp / temp_bytes: LZ4 uses temp only
 * for those derived offsets; LZ4 frames / nvcomp need lzh_decompress_temp_bytes; zstd runs its
 * four-kernel decoder in temp when temp_bytes >= lzh_decompress_temp_bytes (chunks of 16 KiB and more),
 * else every frame in the one-wave decoder (same results, slower); snappy chunks of 512 KiB .. 4 MiB
 * (8..64 fragments of 64 KiB) decode a fragment per wave (split at the tag that starts each fragment,
 * whole where that is not possible) when temp_bytes >= lzh_decompress_temp_bytes, else whole (same
 * results, slower).  d_status: nchunks i32,
 * decoded size per chunk or negative on malformed input (zstd / LZ4 frame / nvcomp container:
 * -1 corrupt, -2 unsupported frame feature).  A chunk whose compressed size equals its size is stored raw (all codecs).
 * Replaces (zstd): lzbench_zstd_decompress, compressors.cpp:1767-1773 (ZSTD_decompressDCtx). */
int lzh_decompress_async(int codec, const void* d_packed, size_t packed_readable, const uint32_t* d_csizes,
                         const uint64_t* d_offsets, size_t n, size_t chunk_size, void* d_out, int32_t* d_status,
                         void* d_temp, size_t temp_bytes, void* hip_stream);

/* ---- 3b. ragged batches ---------------------------------------------------------------- */
/* The calls above with per-chunk pointers and sizes (the shape of the reference's batched calls,
 * nvcomp/lz4.h:292-371) in place of one buffer cut at a chunk size: chunk i is the d_in_bytes[i] bytes at
 * d_in_ptrs[i], any alignment, chunks may overlap or repeat.  d_in_ptrs, d_in_bytes, d_out_ptrs and
 * d_out_bytes are device arrays of nchunks entries; nothing here synchronises with the host or reads a size
 * back, so the calls can be captured in a stream like the uniform ones.
 * Codecs: LZH_CODEC_LZ4 (level = acceleration, as above) and LZH_CODEC_SNAPPY; zstd, the LZ4 frame, the
 * nvcomp container and memcpy return LZH_EARG (so do their sizing functions: 0).  zstd has entry points of
 * its own, section 3c below; the five functions of this section keep refusing LZH_CODEC_ZSTD.
 * Output: as the uniform compress call writes it -- d_csizes[i], d_offsets[0 .. nchunks] ([nchunks] = the packed
 * total), chunks packed contiguously in index order, a chunk whose compressed size equals its size stored raw; equal
 * sizes over contiguous inputs give the uniform call's bytes.  A zero-length chunk is legal (the one-byte LZ4
 * block / snappy varint).  nchunks == 0 returns LZH_OK and launches nothing.
 * Readable slack: every input chunk needs 16 readable bytes after it (the uniform calls' in_readable >= n + 16);
 * the kernels address a chunk through a buffer descriptor of its size + 16 and read nothing past that.
 * max_chunk_bytes bounds every d_in_bytes[i] / d_out_bytes[i]; at most 16 MiB (the sequence records' limit),
 * else LZH_EARG.  A chunk whose device-side size is larger is not processed: compression gives d_csizes[i] = 0
 * (it takes no packed bytes), decompression d_status[i] = -1; no kernel touches that chunk's slots.
 * packed_cap: the sizes are only known on the device, so the capacity is enforced there, as the uniform pack does:
 * a chunk whose packed range would pass packed_cap is not written, d_csizes and d_offsets still report every size,
 * and d_offsets[nchunks] > packed_cap tells the caller that the output is incomplete.
 * lzh_ragged_max_packed_bytes is the capacity no batch of that total size and chunk count exceeds.
 * Temp: nchunks staging slots, then nchunks sequence-record slots, each sized for max_chunk_bytes (compress);
 * scanned offsets and nchunks 32-byte block descriptors (decompress).  One large chunk therefore makes every
 * slot large: a skewed batch pays nchunks x the largest chunk in temp.  The compact calls below size every
 * slot from its own chunk instead.
 * Checks (codec, max_chunk_bytes, null pointers, then temp_bytes below the sizing answer: LZH_ESPACE) come
 * before any device call; the sizing functions are host arithmetic.
 * d_offsets of the decompress call may be NULL (derived from d_csizes into d_temp).  d_status[i]: decoded
 * size of chunk i, negative on malformed input, as above. */
size_t lzh_ragged_compress_temp_bytes(int codec, size_t max_chunk_bytes, size_t nchunks);
size_t lzh_ragged_decompress_temp_bytes(int codec, size_t max_chunk_bytes, size_t nchunks);
size_t lzh_ragged_max_packed_bytes(int codec, size_t total_in_bytes, size_t nchunks);
int lzh_compress_ragged_async(int codec, int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                              size_t nchunks, size_t max_chunk_bytes, void* d_packed, size_t packed_cap,
                              uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp, size_t temp_bytes,
                              void* hip_stream);
int lzh_decompress_ragged_async(int codec, const void* d_packed, size_t packed_readable, const uint32_t* d_csizes,
                                const uint64_t* d_offsets, void* const* d_out_ptrs, const uint64_t* d_out_bytes,
                                size_t nchunks, size_t max_chunk_bytes, int32_t* d_status, void* d_temp,
                                size_t temp_bytes, void* hip_stream);

/* Compact compress layout: lzh_compress_ragged_async with every chunk's staging slot and record slot sized
 * from that chunk's own d_in_bytes[i] (256-aligned) and placed by an exclusive scan on the device, so temp
 * grows with the batch's total bytes (about 3.1 x total for LZ4, 3.2 x for snappy) plus some 600 bytes and the
 * record-count header per chunk, not with nchunks x max_chunk_bytes: 4096 chunks of which one has 16 MiB and
 * the others 4 KiB size to ~100 MiB instead of ~192 GiB.  Codecs, levels, limits, the packed output
 * (d_csizes, d_offsets, the packed bytes, the raw-store rule) and the order of the checks are those of
 * lzh_compress_ragged_async; for a batch that keeps the promise below every output byte equals that call's.
 * The decompress side needs no counterpart (its temp is offsets and descriptors).
 * total_in_bytes: the caller's host-side upper bound of the sum of d_in_bytes[i] over the chunks that are not
 * larger than max_chunk_bytes -- the sizes live on the device and nothing is read back, the packed_cap rule.
 * The sizing function's answer covers every batch of at most nchunks chunks, each of at most max_chunk_bytes,
 * that sums to at most total_in_bytes, and is non-decreasing in each argument; 0 for other codecs or
 * max_chunk_bytes over 16 MiB.  Both functions derive a staging region and a record region from the same three
 * numbers.  On the device a chunk is processed exactly when both of its slots end inside their regions; a
 * chunk that is not (only in a batch that breaks the promise) is handled as a chunk over max_chunk_bytes:
 * d_csizes[i] = 0, no packed bytes, no kernel touches a slot for it.  A chunk over max_chunk_bytes takes
 * slots of 0 bytes.  Every slot is addressed through a buffer descriptor of its own size, so nothing is
 * written outside d_temp[0 .. temp_bytes) whatever the sizes on the device say. */
size_t lzh_ragged_compact_compress_temp_bytes(int codec, size_t total_in_bytes, size_t max_chunk_bytes,
                                              size_t nchunks);
int lzh_compress_ragged_compact_async(int codec, int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                      size_t nchunks, size_t max_chunk_bytes, size_t total_in_bytes, void* d_packed,
                                      size_t packed_cap, uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp,
                                      size_t temp_bytes, void* hip_stream);
/* Host mirror of the compact slot placement for host arrays of sizes (host arithmetic only): stage_off[i] and
 * rec_off[i] = the offsets of chunk i's slots inside the staging region and the record region, processed[i] =
 * 1 when the device processes chunk i.  Returns LZH_OK, or LZH_EARG where the async call would. */
int lzh_debug_ragged_compact_slots(int codec, const uint64_t* sizes, size_t nchunks, size_t max_chunk_bytes,
                                   size_t total_in_bytes, uint64_t* stage_off, uint64_t* rec_off, uint8_t* processed);
/* Debug only, for tests of the placement (no caller needs it; it may change with the temp layout): the two
 * regions both functions derive, as byte ranges of d_temp: out[0], out[1] = offset and size of the
 * staging region, out[2], out[3] = of the record region.  Host arithmetic only; LZH_EARG as above. */
int lzh_debug_ragged_compact_regions(int codec, size_t total_in_bytes, size_t max_chunk_bytes, size_t nchunks,
                                     uint64_t* out);

/* ---- 3c. ragged zstd batches ------------------------------------------------------------ */
/* lzh_compress_ragged_async / lzh_decompress_ragged_async for zstd frames (LZH_CODEC_ZSTD above), under names of
 * their own.  The contract is that of 3b: chunk i is the d_in_bytes[i] bytes at d_in_ptrs[i], any alignment, chunks
 * may overlap or repeat; every input chunk needs 16 readable bytes after it; max_chunk_bytes bounds every
 * d_in_bytes[i] / d_out_bytes[i] and is at most 16 MiB, else LZH_EARG; nchunks == 0 returns LZH_OK and launches
 * nothing; the checks (level / max_chunk_bytes, null pointers, then temp_bytes below the sizing answer:
 * LZH_ESPACE) come before any device call; the sizing functions are host arithmetic and non-decreasing in
 * max_chunk_bytes, nchunks and total_in_bytes.  A chunk whose device-side size is larger than max_chunk_bytes is not
 * processed and no kernel touches its slots: d_csizes[i] = 0 (no packed bytes) on compression, d_status[i] = -1 on
 * decompression.  packed_cap is enforced on the device by the pack kernel (a chunk whose packed range would pass it
 * is not written) and d_offsets[nchunks] > packed_cap reports an incomplete output.  d_offsets of the decompress
 * call may be NULL (derived from d_csizes into d_temp).  A chunk whose compressed size equals its size is stored
 * raw, on both sides.
 * Frame i: chunk i becomes the frame lzbench's zstd row writes for a chunk of that size alone
 * (ZSTD_getParams(level, size, 0), content size, no checksum) -- the bytes lzh_compress_async(LZH_CODEC_ZSTD, level,
 * ..., n = size, chunk_size >= size) writes; equal sizes over contiguous input give the uniform call's d_csizes,
 * d_offsets and packed bytes.  A zero-length chunk is legal: the 9-byte frame of an empty input.
 * Levels: accepted exactly when lzh_level_supported(LZH_CODEC_ZSTD, level, max_chunk_bytes) is 1 (level 2 only for
 * max_chunk_bytes <= 131072: above that some size's row is double-fast); else LZH_EARG, and the compress sizing
 * function returns 0.
 * Compress temp: nchunks staging slots, then nchunks scratch areas of the two zstd kernels (sequences, literals,
 * a block attempt, a Huffman stream, the hash table), every one sized for max_chunk_bytes: nchunks x (the staging
 * stride + the scratch stride of max_chunk_bytes; 1.26 MiB a chunk at 128 KiB, 278 KiB at 16 KiB), so a skewed
 * batch pays for its largest chunk nchunks times; the compact calls at the end of this section size every slot
 * from its own chunk instead.  Decompress temp: the scanned offsets (as 3b); the split decoder's temp below is
 * optional.
 * lzh_zstd_ragged_max_packed_bytes: zstd expands small chunks (1..64 bytes become size + 9, which is not stored
 * raw); the bound is the sum of the per-chunk bounds lzh_stage_stride(LZH_CODEC_ZSTD, .) is sized for.
 * Decoding: any frame of lzbench's shape, also with the content checksum; the verdicts of lzh_decompress_async.
 * Which decoder runs follows that call's rule, by temp_bytes.  With lzh_zstd_ragged_decompress_temp_bytes every
 * frame decodes in the one-wave decoder.  With at least lzh_zstd_ragged_decompress_split_temp_bytes, where that is
 * not 0, the four-kernel split decoder runs (header, Huffman literals, sequences a frame per lane, execution) and
 * the one-wave decoder takes only the frames it leaves: same statuses and bytes, several times faster on batches of
 * many frames.  That answer is 0 for max_chunk_bytes below 16384 or above 16 MiB (no split decoder:
 * pass the other size); otherwise it is the uniform decoder's layout for nchunks frames of max_chunk_bytes after the
 * scanned offsets -- per frame the block, table and sequence-record areas (about 280 KiB a frame at 128 KiB), then
 * frame states, frame fields and Huffman jobs -- so a skewed batch again pays for its largest chunk nchunks times.
 * It is host arithmetic, non-decreasing in both arguments and never below the other answer; a temp_bytes between
 * the two decodes one-wave.  A chunk whose device-side size passes max_chunk_bytes is left alone by both decoders
 * (d_status[i] = -1), its temp slot included.
 * Streams: every launch goes on hip_stream, with either temp -- no side stream, event, plan kernel, host
 * synchronisation or size read back (the uniform zstd calls fork to side streams) -- so a captured call has no
 * parallel branches. */
size_t lzh_zstd_ragged_compress_temp_bytes(int level, size_t max_chunk_bytes, size_t nchunks);
size_t lzh_zstd_ragged_decompress_temp_bytes(size_t max_chunk_bytes, size_t nchunks);
size_t lzh_zstd_ragged_decompress_split_temp_bytes(size_t max_chunk_bytes, size_t nchunks);
size_t lzh_zstd_ragged_max_packed_bytes(size_t total_in_bytes, size_t nchunks);
int lzh_zstd_compress_ragged_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                   size_t nchunks, size_t max_chunk_bytes, void* d_packed, size_t packed_cap,
                                   uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp, size_t temp_bytes,
                                   void* hip_stream);
int lzh_zstd_decompress_ragged_async(const void* d_packed, size_t packed_readable, const uint32_t* d_csizes,
                                     const uint64_t* d_offsets, void* const* d_out_ptrs, const uint64_t* d_out_bytes,
                                     size_t nchunks, size_t max_chunk_bytes, int32_t* d_status, void* d_temp,
                                     size_t temp_bytes, void* hip_stream);
/* Debug only, for tests (it may change with the temp layout): the regions of the split decoder's temp as byte
 * ranges of d_temp, out[2 i], out[2 i + 1] = offset and size of region i: 0 scanned offsets, 1 per-frame areas
 * (nchunks of out[14] bytes each), 2 the sequence waves' dummy words, 3 frame states (nchunks x i32: 2 = finished
 * by the split kernels or not processed, 1 = handed to the one-wave decoder), 4 frame fields, 5 the Huffman jobs'
 * counter, 6 the Huffman jobs; out[14] = a frame area's size, out[15] = the sizing answer (16 values).  Host
 * arithmetic only; LZH_EARG where the sizing answer is 0 or out is null. */
int lzh_debug_zstd_ragged_split_layout(size_t max_chunk_bytes, size_t nchunks, uint64_t* out);

/* Compact compress layout: lzh_zstd_compress_ragged_async with every chunk's staging slot and scratch slot sized
 * from that chunk's own d_in_bytes[i] and the level (256-aligned) and placed by an exclusive scan on the device,
 * so temp grows with the batch's total bytes plus a constant per chunk, not with nchunks x (the slots of
 * max_chunk_bytes).  A chunk of n bytes takes a staging slot of lzh_stage_stride(LZH_CODEC_ZSTD, n) and a
 * scratch slot of what the two zstd kernels address for a frame of that size alone: about 8 x min(n, 128 KiB)
 * + 6.5 KiB for sequences, literals, the block attempt and a Huffman stream, and the frame's own hash table
 * (4 << hashLog bytes: up to 16 x n for a small chunk, at most 256 KiB; not monotone in n, since hashLog drops
 * where n enters the next size class of ZSTD_getParams).  An empty chunk takes the slots of a 1-byte chunk
 * (6912 bytes of scratch; it touches the first 1024).  The scratch region is sized as the smaller of
 * nchunks x the largest slot of any size up to max_chunk_bytes at that level and the sum of three bounds: the
 * areas before the table, min(8 x total_in_bytes, nchunks x 8 x min(max_chunk_bytes, 128 KiB)) -- one large
 * chunk pays for one block, not for its size -- 6656 bytes a chunk, and the tables, min(16 x total_in_bytes
 * + 512 x nchunks, nchunks x the largest table up to max_chunk_bytes); the staging region as the smaller of
 * total + total / 256 + 335 x nchunks and nchunks x the slot of max_chunk_bytes.  The sizing function's own
 * answers:
 *   4096 chunks, one of 16 MiB and 4095 of 4 KiB (33,550,336 bytes in all):   867,689,472 bytes (0.81 GiB) at
 *       level 1 and 465,036,288 (0.43 GiB) at level -1, where lzh_zstd_ragged_compress_temp_bytes answers
 *       74,381,787,648 (69.27 GiB);
 *   4096 chunks of 128 KiB:   5,396,071,424 bytes (5.03 GiB) at level 1 against 5,395,972,608 -- a uniform batch
 *       gains nothing there (the same slots and the four arrays, 98,816 bytes) and only the level's own hash
 *       table elsewhere (level -1: 4,993,418,240; the uniform-slot layout takes the worst level's).
 * Levels, the 16 MiB limit, zero-length chunks, the packed output (d_csizes, d_offsets, the packed bytes, the
 * raw-store rule), packed_cap enforced on the device, the streams (every launch on hip_stream) and the order of
 * the checks (level / max_chunk_bytes, nchunks == 0: LZH_OK, null pointers, then temp_bytes: LZH_ESPACE) are
 * those of lzh_zstd_compress_ragged_async; for a batch that keeps the promise below d_csizes, d_offsets and every
 * packed byte equal that call's.
 * total_in_bytes: the caller's host-side upper bound of the sum of d_in_bytes[i] over the chunks that are not
 * larger than max_chunk_bytes -- the sizes live on the device and nothing is read back, the packed_cap rule.
 * The sizing function's answer covers every batch of at most nchunks chunks, each of at most max_chunk_bytes,
 * that sums to at most total_in_bytes; it is non-decreasing in each of the three, never above
 * lzh_zstd_ragged_compress_temp_bytes(level, max_chunk_bytes, nchunks) plus the four per-chunk arrays (two u32,
 * two u64 of nchunks + 1), and 0 where that function answers 0.  Both functions derive a staging region and a
 * scratch region from the same four numbers.  On the device a chunk is processed exactly when it is at most
 * max_chunk_bytes and both of its slots end inside their regions; a chunk that is not (the second case only in a
 * batch that breaks the promise) gets d_csizes[i] = 0, takes no packed bytes, and no kernel touches a slot for it.
 * A chunk over max_chunk_bytes takes slots of 0 bytes.  Every slot is addressed through buffer descriptors
 * bounded by the slot, so nothing is written outside d_temp[0 .. temp_bytes) whatever the sizes on the device say.
 * Decompression needs no counterpart: lzh_zstd_decompress_ragged_async's small temp is the scanned offsets, and
 * the split decoder's temp stays sized per largest chunk (not addressed here). */
size_t lzh_zstd_ragged_compact_compress_temp_bytes(int level, size_t total_in_bytes, size_t max_chunk_bytes,
                                                   size_t nchunks);
int lzh_zstd_compress_ragged_compact_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                           size_t nchunks, size_t max_chunk_bytes, size_t total_in_bytes,
                                           void* d_packed, size_t packed_cap, uint32_t* d_csizes, uint64_t* d_offsets,
                                           void* d_temp, size_t temp_bytes, void* hip_stream);
/* Host mirror of the compact slot placement for host arrays of sizes (host arithmetic only): stage_off[i] and
 * scratch_off[i] = the offsets of chunk i's slots inside the staging region and the scratch region, processed[i]
 * = 1 when the device processes chunk i.  Returns LZH_OK, or LZH_EARG where the async call would. */
int lzh_debug_zstd_ragged_compact_slots(int level, const uint64_t* sizes, size_t nchunks, size_t max_chunk_bytes,
                                        size_t total_in_bytes, uint64_t* stage_off, uint64_t* scratch_off,
                                        uint8_t* processed);
/* Debug only, for tests of the placement (it may change with the temp layout): the two regions as byte ranges of
 * d_temp: out[0], out[1] = offset and size of the staging region, out[2], out[3] = of the scratch region.  Host
 * arithmetic only; LZH_EARG as above. */
int lzh_debug_zstd_ragged_compact_regions(int level, size_t total_in_bytes, size_t max_chunk_bytes, size_t nchunks,
                                          uint64_t* out);

/* ---- 3d. LZ4 ragged batches with a shared dictionary ------------------------------------- */
/* lzh_compress_ragged_async / lzh_decompress_ragged_async for LZ4 with one dictionary shared by every chunk of the
 * batch: what LZ4_loadDict + LZ4_compress_fast_continue and LZ4_decompress_safe_usingDict do for small records
 * (256 bytes to some KiB), which alone find little to match.  The contract is that of 3b -- device arrays of nchunks
 * entries, any alignment, chunks may overlap or repeat, 16 readable bytes after every input chunk, nchunks == 0
 * returns LZH_OK and launches nothing, a chunk larger than max_chunk_bytes is not processed (d_csizes[i] = 0 /
 * d_status[i] = -1), packed_cap enforced on the device, d_offsets of the decompress call may be NULL, the raw-store
 * rule on both sides, the packed layout (d_csizes, d_offsets[0 .. nchunks], chunks contiguous in index order: the
 * scan and the pack are those of lzh_compress_ragged_async) -- but for the dictionary arguments and the limits:
 *   d_dict, dict_bytes: the dictionary, one device buffer of any alignment with 16 readable bytes after it;
 *       8 <= dict_bytes <= 65536, else LZH_EARG (below 8 bytes LZ4_loadDict loads nothing; a longer dictionary is
 *       the caller's to cut to its last 64 KiB, as LZ4_loadDict does);
 *   max_chunk_bytes <= 4 MiB, else LZH_EARG.
 * The sizing functions return 0 exactly where the calls return LZH_EARG for those arguments; they are host
 * arithmetic and non-decreasing in every argument.  Check order: arguments, nchunks == 0, null pointers (d_dict
 * among them), then temp_bytes below the sizing answer: LZH_ESPACE; all before any device call.
 * Compressed bytes: chunk i is exactly what lz4 1.9.3 writes for it when the dictionary lies directly before the
 * chunk in one buffer, a fresh LZ4_stream_t gets LZ4_loadDict(stream, dict, dict_bytes), and
 * LZ4_compress_fast_continue(stream, chunk, dst, n, LZ4_compressBound(n), acc) runs, acc = level (level <= 1: 1).
 * Decoding: d_status[i] and the bytes are those of LZ4_decompress_safe_usingDict(src, dst, csize, d_out_bytes[i],
 * dict, dict_bytes): the decoded size, or negative where the reference returns negative; an offset may reach
 * dict_bytes before the chunk's first byte, one more is an error; blocks written without a dictionary decode as
 * before.
 * Temp: nchunks staging slots of lzh_stage_stride(LZH_CODEC_LZ4, max_chunk_bytes) and the dictionary's hash table
 * (16 KiB, built once per call) for compression -- never above lzh_ragged_compress_temp_bytes(LZH_CODEC_LZ4, ..)
 * + 64 KiB + 64 bytes a chunk, and no copy of the dictionary; the scanned offsets for decompression.
 * Streams: every launch goes on hip_stream; no side stream, event, host synchronisation or size read back. */
size_t lzh_lz4_dict_compress_temp_bytes(size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks);
size_t lzh_lz4_dict_decompress_temp_bytes(size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks);
int lzh_lz4_compress_ragged_dict_async(int level, const void* d_dict, size_t dict_bytes,
                                       const void* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t nchunks,
                                       size_t max_chunk_bytes, void* d_packed, size_t packed_cap, uint32_t* d_csizes,
                                       uint64_t* d_offsets, void* d_temp, size_t temp_bytes, void* hip_stream);
int lzh_lz4_decompress_ragged_dict_async(const void* d_dict, size_t dict_bytes, const void* d_packed,
                                         size_t packed_readable, const uint32_t* d_csizes, const uint64_t* d_offsets,
                                         void* const* d_out_ptrs, const uint64_t* d_out_bytes, size_t nchunks,
                                         size_t max_chunk_bytes, int32_t* d_status, void* d_temp, size_t temp_bytes,
                                         void* hip_stream);

/* ---- 3e. ragged zstd level-3 batches (the double-fast strategy) ------------------------- */
/* lzh_zstd_compress_ragged_async and lzh_zstd_compress_ragged_compact_async for zstd level 3 (LZH_CODEC_ZSTD_DFAST
 * above), under names of their own: the calls of 3b keep refusing the codec and those of 3c the level.  The contract
 * is that of 3c, word for word -- device arrays of nchunks entries, chunk i the d_in_bytes[i] bytes at d_in_ptrs[i],
 * any alignment, chunks may overlap or repeat; 16 readable bytes after every input chunk; max_chunk_bytes at most
 * 16 MiB, else LZH_EARG; nchunks == 0 returns LZH_OK and launches nothing; a chunk whose device-side size is larger
 * than max_chunk_bytes is not processed and no kernel touches its slots (d_csizes[i] = 0, no packed bytes);
 * packed_cap is enforced on the device by the pack kernel and d_offsets[nchunks] > packed_cap reports an incomplete
 * output; a chunk whose compressed size equals its size is stored raw; the order of the checks (level /
 * max_chunk_bytes, nchunks == 0: LZH_OK, null pointers, then temp_bytes below the sizing answer: LZH_ESPACE), all
 * before any device call; every launch on hip_stream, no side stream, event, host synchronisation or size read
 * back, so a captured call has no parallel branches -- with these exceptions:
 *   level must be 3: any other level returns LZH_EARG, and the two sizing functions return 0 for it (as they do
 *       for max_chunk_bytes above 16 MiB);
 *   frame i is the bytes lzh_compress_async(LZH_CODEC_ZSTD_DFAST, 3, ..., n = size, chunk_size >= size) writes --
 *       ZSTD_getParams(3, size, 0), content size, no checksum; equal sizes over contiguous input give the uniform
 *       call's d_csizes, d_offsets and packed bytes.  A zero-length chunk is legal: the 9-byte frame.
 * Uniform-slot temp: nchunks x (lzh_stage_stride(LZH_CODEC_ZSTD, max_chunk_bytes) + the level-3 scratch stride of
 * max_chunk_bytes), exactly (no spare bytes; so 0 for nchunks == 0, where the call launches nothing and needs no
 * temp), a batch of empty chunks laid out as one of 1-byte chunks.  The scratch stride is the
 * areas of 3c (about 8 x min(max_chunk_bytes, 128 KiB) + 6.5 KiB) and the two double-fast tables, the long one of
 * 4 << hashLog and the short one of 4 << chainLog bytes, each the largest of any size up to max_chunk_bytes (768 KiB
 * above 256 KiB chunks): 1,447,680 bytes at 128 KiB (1.51 MiB a chunk with the staging slot), 350,208 a chunk at
 * 16 KiB.
 * Compact temp (lzh_zstd_dfast_compress_ragged_compact_async): every chunk's staging slot and scratch slot sized from
 * that chunk's own d_in_bytes[i] (256-aligned) and placed by an exclusive scan on the device, the promise of
 * total_in_bytes, the rule for a chunk whose slots end outside their regions (d_csizes[i] = 0, nothing touched) and
 * the descriptor bounds as in 3c.  A chunk of n bytes takes a staging slot of lzh_stage_stride(LZH_CODEC_ZSTD, n) and
 * a scratch slot of the areas for its own block size plus its own two tables (ZSTD_getParams(3, n, 0): under 24 x n
 * from 64 bytes on, 768 bytes below; 48 KiB for a chunk of 4 KiB); an empty chunk takes the slots of a 1-byte chunk.
 * The scratch region is the smaller of nchunks x the uniform-slot scratch stride and the sum of three bounds:
 * min(8 x total_in_bytes, nchunks x 8 x min(max_chunk_bytes, 128 KiB)), 6656 bytes a chunk, and the tables,
 * min(24 x total_in_bytes + 768 x nchunks, nchunks x the largest two tables up to max_chunk_bytes); the staging
 * region as in 3c.  The answer covers every batch of at most nchunks chunks, each of at most max_chunk_bytes, that
 * sums to at most total_in_bytes; it is non-decreasing in each of the three and never above
 * lzh_zstd_dfast_ragged_compress_temp_bytes(3, max_chunk_bytes, nchunks) plus the four per-chunk arrays (two u32 of
 * nchunks, two u64 of nchunks + 1, each 256-aligned).  The sizing function's own answers, next to 3c's:
 *   4096 chunks, one of 16 MiB and 4095 of 4 KiB (33,550,336 bytes in all):   1,139,171,840 bytes (1.06 GiB; level 1
 *       in 3c: 867,689,472), where lzh_zstd_dfast_ragged_compress_temp_bytes answers 76,529,270,784 (71.27 GiB);
 *   4096 chunks of 128 KiB:   6,469,812,736 bytes (6.03 GiB) against 6,469,713,920 -- a uniform batch gains nothing
 *       (the same slots and the four arrays, 98,816 bytes).
 * Decoding: no call of its own.  These are LZH_CODEC_ZSTD's frames and decode with lzh_zstd_decompress_ragged_async,
 * in the one-wave or the four-kernel split decoder by that call's temp_bytes
 * (lzh_zstd_ragged_decompress_temp_bytes / lzh_zstd_ragged_decompress_split_temp_bytes);
 * lzh_zstd_ragged_max_packed_bytes bounds the packed output (the frames have LZH_CODEC_ZSTD's bound).
 * The two debug calls are those of 3c for this layout (host arithmetic only; LZH_EARG where the async call would
 * return it, or for a null pointer): the host mirror of the slot placement, and the two regions as byte ranges of
 * d_temp, out[0], out[1] = offset and size of the staging region, out[2], out[3] = of the scratch region. */
size_t lzh_zstd_dfast_ragged_compress_temp_bytes(int level, size_t max_chunk_bytes, size_t nchunks);
int lzh_zstd_dfast_compress_ragged_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                         size_t nchunks, size_t max_chunk_bytes, void* d_packed, size_t packed_cap,
                                         uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp, size_t temp_bytes,
                                         void* hip_stream);
size_t lzh_zstd_dfast_ragged_compact_compress_temp_bytes(int level, size_t total_in_bytes, size_t max_chunk_bytes,
                                                         size_t nchunks);
int lzh_zstd_dfast_compress_ragged_compact_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                                 size_t nchunks, size_t max_chunk_bytes, size_t total_in_bytes,
                                                 void* d_packed, size_t packed_cap, uint32_t* d_csizes,
                                                 uint64_t* d_offsets, void* d_temp, size_t temp_bytes, void* hip_stream);
int lzh_debug_zstd_dfast_ragged_compact_slots(int level, const uint64_t* sizes, size_t nchunks, size_t max_chunk_bytes,
                                              size_t total_in_bytes, uint64_t* stage_off, uint64_t* scratch_off,
                                              uint8_t* processed);
int lzh_debug_zstd_dfast_ragged_compact_regions(int level, size_t total_in_bytes, size_t max_chunk_bytes,
                                                size_t nchunks, uint64_t* out);

/* ---- 3f. ragged zstd batches with a shared dictionary ------------------------------------- */
/* lzh_zstd_compress_ragged_async / lzh_zstd_decompress_ragged_async with one raw-content dictionary shared by every
 * chunk of the batch: what ZSTD_compress_usingDict and ZSTD_decompress_usingDict do for small records (pages, log
 * lines, column chunks), which alone find little to match -- 1,000 bytes of word text: 566 bytes alone, 379 with a
 * 4 KiB dictionary of the same vocabulary (level 1).  The contract is that of 3c, word for word -- device arrays of
 * nchunks entries, any alignment, chunks may overlap or repeat; 16 readable bytes after every input chunk; nchunks == 0
 * returns LZH_OK and launches nothing; a chunk whose device-side size is larger than max_chunk_bytes is not processed
 * and no kernel touches a slot for it (d_csizes[i] = 0 / d_status[i] = -1); packed_cap enforced on the device by the
 * pack kernel; d_offsets of the decompress call may be NULL; the raw-store rule on both sides; the packed layout, the
 * scan and the pack of lzh_zstd_compress_ragged_async; every launch on hip_stream, no side stream, event, host
 * synchronisation or size read back -- but for the dictionary arguments and the limits:
 *   d_dict, dict_bytes: the dictionary, one device buffer of any alignment with 16 readable bytes after it;
 *       8 <= dict_bytes <= 131072, else LZH_EARG (below 8 bytes the reference loads nothing; 131072 covers zstd's
 *       default trained size of 112,640 bytes).  The bytes are always used as content: a buffer that begins with
 *       zstd's dictionary magic (37 A4 30 EC) would be parsed by the reference as a trained dictionary with entropy
 *       tables, and this call does not do that -- trained dictionaries are out of scope;
 *   max_chunk_bytes <= 131072, else LZH_EARG: dictionary plus chunk never pass 256 KiB, every frame has one block
 *       inside its window and the dictionary is never invalidated mid-frame;
 *   level: 1 and -1 .. -5, the levels whose row is ZSTD_fast in all four tables, else LZH_EARG (level 3,
 *       double-fast with a dictionary, is the call of 3h; level 2 is not built).
 * The sizing functions return 0 exactly where the calls return LZH_EARG for those arguments; they are host arithmetic
 * and non-decreasing in dict_bytes, max_chunk_bytes and nchunks (and the same for every accepted level).  Check order:
 * arguments, nchunks == 0, null pointers (d_dict among them), then temp_bytes below the sizing answer: LZH_ESPACE; all
 * before any device call.
 * Compressed bytes: frame i is exactly what zstd 1.5.2 writes for ZSTD_compress_usingDict(cctx, dst, cap, chunk, n,
 * dict, dict_bytes, level) on a fresh ZSTD_CCtx when the dictionary lies in a buffer of its own, not directly before
 * the chunk (adjacent, the reference runs its prefix parser and the bytes differ from about 300-byte chunks on):
 * ZSTD_getParams_internal(level, n, dict_bytes) -- the row by n + dict_bytes, the window cut to ceil log2 of it --
 * ZSTD_loadDictionaryContent's table fill, ZSTD_compressBlock_fast_extDict_generic, and the frame of 3c (content
 * size, no checksum, dictionary id 0 and so no id field, single segment).  A chunk under 7 bytes gives the bytes of
 * the plain call, an empty one the 9-byte frame.
 * Decoding: d_status[i] and the bytes are those of ZSTD_decompress_usingDict(dctx, dst, d_out_bytes[i], src, csize,
 * dict, dict_bytes) for any frame of lzbench's shape, also one no encoder here writes (the reference at levels 3, 5,
 * 19 with the dictionary): an offset may reach dict_bytes before the chunk's first byte, one more gives -1; a match
 * may start in the dictionary and run on into the output; frames written without a dictionary decode as before; a
 * frame with a dictionary id field reports -2.  The one-wave decoder only: no split temp is accepted.
 * Temp: nchunks staging slots of lzh_stage_stride(LZH_CODEC_ZSTD, max_chunk_bytes), nchunks scratch areas (the areas
 * of 3c for a block of max_chunk_bytes and the frame's own copy of the dictionary's table: 4 << hashLog bytes, the
 * largest any frame of such a batch can take, 128 KiB once dictionary plus chunk pass 8 KiB), and one filled table per
 * (hashLog, minMatch) class a batch can take, built once per call (a constant 359,936 bytes); the scanned offsets for
 * decompression.
 * The two debug calls are host arithmetic only: lzh_debug_zstd_dict_params writes windowLog, hashLog, minMatch,
 * targetLength and the block size of ZSTD_getParams(level, n, dict_bytes) to out[0 .. 5); lzh_debug_zstd_dict_parse
 * walks the parse on the host (host pointers, 16 readable bytes after each) and writes the first cap sequences as
 * (literal length, match length, offBase) triples, returning the count; LZH_EARG where the async call would return it
 * (n taking max_chunk_bytes' place) or for a null pointer. */
size_t lzh_zstd_dict_compress_temp_bytes(int level, size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks);
size_t lzh_zstd_dict_decompress_temp_bytes(size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks);
int lzh_zstd_compress_ragged_dict_async(int level, const void* d_dict, size_t dict_bytes,
                                        const void* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t nchunks,
                                        size_t max_chunk_bytes, void* d_packed, size_t packed_cap, uint32_t* d_csizes,
                                        uint64_t* d_offsets, void* d_temp, size_t temp_bytes, void* hip_stream);
int lzh_zstd_decompress_ragged_dict_async(const void* d_dict, size_t dict_bytes, const void* d_packed,
                                          size_t packed_readable, const uint32_t* d_csizes, const uint64_t* d_offsets,
                                          void* const* d_out_ptrs, const uint64_t* d_out_bytes, size_t nchunks,
                                          size_t max_chunk_bytes, int32_t* d_status, void* d_temp, size_t temp_bytes,
                                          void* hip_stream);
int lzh_debug_zstd_dict_params(int level, size_t n, size_t dict_bytes, uint32_t* out);
long lzh_debug_zstd_dict_parse(int level, const void* dict, size_t dict_bytes, const void* src, size_t n,
                               uint32_t* seqs, size_t cap);

/* Debug only, host arithmetic only (they may change; the call that decodes through this layout and its sizing
 * function are section 3g below): a compact layout of the split
 * decoder's temp, in which every frame's area is laid out for that frame's own decoded size and placed by an
 * exclusive scan, and the Huffman job list is sized for the sum of the frames' own block slots, so temp grows with the
 * batch's total bytes plus a constant per chunk, not with nchunks x (the area of max_chunk_bytes).  A frame of n
 * bytes takes ceil(n / 128 KiB) + 1 block slots of 8,760 bytes (a block's fields, its sequence tables and its Huffman
 * table) and n / 4 + 64 sequence records of 8 bytes, 256-aligned (26,368 bytes at 4 KiB, 34,685,184 at 16 MiB), and
 * as many Huffman job slots as block slots.  The area region is the smaller of nchunks x the area of max_chunk_bytes
 * and 2 x total_out_bytes + 8,760 x (total_out_bytes / 131072 + 2 x nchunks) + 767 x nchunks; the job list the
 * smaller of nchunks x the block slots of max_chunk_bytes and total_out_bytes / 131072 + 2 x nchunks jobs.
 * total_out_bytes: an upper bound of the sum of the decoded sizes over the chunks not larger than max_chunk_bytes (the
 * promise of total_in_bytes above).  The layout's total (out[22] below) covers every batch of at most nchunks
 * chunks, each of at most max_chunk_bytes, that sums to at most total_out_bytes; it is non-decreasing in each of the
 * three and never above lzh_zstd_ragged_decompress_split_temp_bytes(max_chunk_bytes, nchunks) plus the four per-chunk
 * arrays (two u32 of nchunks, two u64 of nchunks + 1).  Its own answers:
 *   4096 chunks, one of 16 MiB and 4095 of 4 KiB (33,550,336 bytes in all):   145,583,104 bytes, where
 *       lzh_zstd_ragged_decompress_split_temp_bytes answers 142,105,035,776;
 *   4096 chunks of 128 KiB (536,870,912 bytes in all):   1,149,519,360 bytes against 1,149,420,544 -- a uniform
 *       batch gains nothing (the same areas and jobs, and the four arrays).
 * lzh_debug_zstd_ragged_split_compact_layout: the regions as byte ranges, out[2 i], out[2 i + 1] = offset and size
 * of region i: 0 scanned offsets, 1 the area region, 2 the sequence waves' dummy words, 3 frame states (nchunks x
 * i32), 4 frame fields, 5 the Huffman jobs' counter, 6 the Huffman jobs, 7 area sizes, 8 job counts (u32 each), 9 area
 * offsets, 10 job offsets (nchunks + 1 u64 each); out[22] = the total (23 values).  LZH_EARG where
 * lzh_zstd_ragged_decompress_split_temp_bytes answers 0 (max_chunk_bytes below 16384 or above 16 MiB) or out is null.
 * lzh_debug_zstd_ragged_split_compact_slots: the placement for a host array of decoded sizes: area_off[i] = the
 * offset of frame i's area inside the area region, job_off[i] = its first slot in the job list (exclusive scans; a
 * chunk over max_chunk_bytes takes 0 bytes and 0 slots), in_split[i] = 1 exactly when the chunk is at most
 * max_chunk_bytes, its area ends inside the area region and its job slots end inside the job list.  LZH_EARG as above,
 * or for a null pointer with nchunks > 0. */
int lzh_debug_zstd_ragged_split_compact_slots(const uint64_t* out_sizes, size_t nchunks, size_t max_chunk_bytes,
                                              size_t total_out_bytes, uint64_t* area_off, uint64_t* job_off,
                                              uint8_t* in_split);
int lzh_debug_zstd_ragged_split_compact_layout(size_t total_out_bytes, size_t max_chunk_bytes, size_t nchunks,
                                               uint64_t* out);

/* ---- 3g. ragged zstd batches: the split decoder with temp sized by the batch's total bytes ---------------- */
/* lzh_zstd_decompress_ragged_async (3c) through the four-kernel split decoder in the compact temp layout described
 * above: every frame's area laid out for the frame's own decoded size and placed on the device by an exclusive scan,
 * the Huffman job list sized for the sum of the frames' own block slots.  A batch of one 16 MiB chunk among 4,095 of
 * 4 KiB decodes in the split decoder with 145,583,104 bytes of temp, where 3c's split temp is 142,105,035,776.
 * lzh_zstd_ragged_decompress_split_compact_temp_bytes: host arithmetic, exactly out[22] of
 * lzh_debug_zstd_ragged_split_compact_layout for the same arguments, and 0 where that call returns LZH_EARG
 * (max_chunk_bytes below 16384 or above 16 MiB): non-decreasing in each argument, never above
 * lzh_zstd_ragged_decompress_split_temp_bytes(max_chunk_bytes, nchunks) plus the four per-chunk arrays.
 * lzh_zstd_decompress_ragged_split_compact_async: the contract of lzh_zstd_decompress_ragged_async, word for word --
 * per-chunk pointers and sizes of any alignment; d_offsets may be NULL (derived into temp); raw-stored chunks are
 * copied; a chunk over max_chunk_bytes is not processed (d_status[i] = -1, nothing of its frame read, nothing of its
 * output or temp written); nchunks == 0 returns LZH_OK and launches nothing; all checks before any device call, in
 * this order: max_chunk_bytes over 16 MiB -> LZH_EARG, nchunks == 0, null pointers -> LZH_EARG, temp_bytes below
 * lzh_zstd_ragged_decompress_temp_bytes -> LZH_ESPACE; every launch on hip_stream, no side stream, event, host
 * synchronisation or size read back -- with one addition: total_out_bytes, the caller's host-side upper bound of the
 * sum of d_out_bytes[i] over the chunks not larger than max_chunk_bytes (the promise the compact compress calls take).
 * The decoder is chosen by temp_bytes as in 3c: with at least the compact sizing answer (where that is not 0) the
 * split decoder runs in the compact layout; with less, every frame decodes in the one-wave decoder.  Statuses and
 * bytes are the same either way, and the same as lzh_zstd_decompress_ragged_async's with either of its temps.
 * Placement: a frame of d_out_bytes[i] = n takes the area and the job slots of a frame of n bytes (above; a chunk over
 * max_chunk_bytes 0 of each), both placed by exclusive scans into regions 7 .. 10 of the layout;
 * lzh_debug_zstd_ragged_split_compact_slots is the host mirror, bit for bit.  A frame within max_chunk_bytes whose area
 * or job slots end outside their regions -- possible only in a batch that breaks the promise -- is not refused: it
 * decodes in the one-wave decoder, so a broken promise costs speed and never a result, and nothing is written outside
 * d_temp[0 .. temp_bytes).  So does a frame of more blocks than ceil(n / 128 KiB) + 1 (its own block slots).
 * The debug hooks lzh_debug_zstd_legacy, lzh_debug_zstd_huf_sections and lzh_debug_zstd_hufpar act as on 3c's call. */
size_t lzh_zstd_ragged_decompress_split_compact_temp_bytes(size_t total_out_bytes, size_t max_chunk_bytes,
                                                           size_t nchunks);
int lzh_zstd_decompress_ragged_split_compact_async(const void* d_packed, size_t packed_readable,
        const uint32_t* d_csizes, const uint64_t* d_offsets, void* const* d_out_ptrs, const uint64_t* d_out_bytes,
        size_t nchunks, size_t max_chunk_bytes, size_t total_out_bytes, int32_t* d_status,
        void* d_temp, size_t temp_bytes, void* hip_stream);

/* ---- 3h. ragged zstd level-3 batches with a shared dictionary ------------------------------ */
/* 3f's compress call at zstd's default level: what ZSTD_compress_usingDict(.., ZSTD_CLEVEL_DEFAULT) does for small
 * records.  The contract is 3f's, word for word -- the dictionary arguments (one device buffer of any alignment, 16
 * readable bytes after it, always used as content), per-chunk pointers and sizes, 16 readable bytes after every
 * chunk, a chunk over max_chunk_bytes not processed (d_csizes[i] = 0, no slot touched), packed_cap enforced by the
 * pack kernel, the raw-store rule, every launch on hip_stream with no side stream, event, host synchronisation or
 * size read back -- with these differences:
 *   level: 3 alone, else LZH_EARG (3f keeps refusing level 3, the calls of 3e keep having no dictionary);
 *   limits: 8 <= dict_bytes <= 131072 and max_chunk_bytes <= 131072, else LZH_EARG;
 *   check order: arguments, nchunks == 0 (LZH_OK, nothing launched), null pointers (d_dict among them), the launch
 *       grid, then temp_bytes below the sizing answer: LZH_ESPACE; all before any device call.
 * Compressed bytes: frame i is exactly what zstd 1.5.2 writes for ZSTD_compress_usingDict(fresh cctx, dst, cap,
 * chunk i, n, dict, dict_bytes, 3) with the dictionary in a buffer of its own (not directly before the chunk):
 * ZSTD_getParams_internal(3, n, dict_bytes) -- level 3's row by n + dict_bytes, adjusted for n + dict_bytes --
 * ZSTD_fillDoubleHashTable(ZSTD_dtlm_fast) over the dictionary, ZSTD_compressBlock_doubleFast_extDict_generic, and the
 * frame of 3e.  A chunk under 7 bytes gives the bytes of the plain call, an empty one the 9-byte frame.
 * Decoding: lzh_zstd_decompress_ragged_dict_async of 3f, unchanged.
 * lzh_zstd_dfast_dict_compress_temp_bytes: 0 exactly where the call returns LZH_EARG for those arguments; host
 * arithmetic, non-decreasing in dict_bytes, max_chunk_bytes and nchunks.  Temp: nchunks staging slots of
 * lzh_stage_stride(LZH_CODEC_ZSTD, max_chunk_bytes), nchunks scratch areas (the areas of 3c for a block of
 * max_chunk_bytes and the frame's private pair of tables, (4 << hashLog) + (4 << chainLog) bytes, the largest any
 * frame of such a batch can take: 512 KiB once dictionary plus chunk pass 32 KiB), and one filled pair of tables per
 * (hashLog, chainLog, minMatch) class a batch can take, built once per call (a constant 1,309,952 bytes).
 * The two debug calls are host arithmetic only: lzh_debug_zstd_dfast_dict_params writes windowLog, hashLog, chainLog,
 * minMatch and the block size of ZSTD_getParams(3, n, dict_bytes) to out[0 .. 5); lzh_debug_zstd_dfast_dict_parse
 * walks the parse on the host (host pointers, 16 readable bytes after each), writes the first cap sequences as
 * (literal length, match length, offBase) triples and returns the count; where events is not null it adds to 14
 * counters of the branches the walk reached, source in the dictionary / in the chunk: [0, 1] repcode at ip + 1,
 * [2, 3] long match, [4, 5] short match kept, [6, 7] long match at ip + 1 taken, [8, 9] offset_2 loop iteration,
 * [10] a forward count that crossed from the dictionary's end into the chunk's start, [11] a catch-up that stopped at
 * the dictionary's first byte, [12] one that stopped at the chunk's first byte, [13] a repcode candidate refused by
 * the three-byte overlap test.  LZH_EARG where the async call would return it (n taking max_chunk_bytes' place) or for
 * a null pointer. */
size_t lzh_zstd_dfast_dict_compress_temp_bytes(int level, size_t dict_bytes, size_t max_chunk_bytes, size_t nchunks);
int lzh_zstd_dfast_compress_ragged_dict_async(int level, const void* d_dict, size_t dict_bytes,
                                              const void* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t nchunks,
                                              size_t max_chunk_bytes, void* d_packed, size_t packed_cap,
                                              uint32_t* d_csizes, uint64_t* d_offsets, void* d_temp, size_t temp_bytes,
                                              void* hip_stream);
int lzh_debug_zstd_dfast_dict_params(int level, size_t n, size_t dict_bytes, uint32_t* out);
long lzh_debug_zstd_dfast_dict_parse(int level, const void* dict, size_t dict_bytes, const void* src, size_t n,
                                     uint32_t* seqs, size_t cap, uint64_t* events);

/* ---- 3i. ragged LZ4 frames -------------------------------------------------------------------- */
/* lzh_compress_ragged_async / lzh_decompress_ragged_async for LZ4 frames (LZH_CODEC_LZ4F above), under names of their
 * own: one self-describing frame per chunk, what the lz4 tool and every LZ4 binding read.  The five functions of 3b
 * keep refusing LZH_CODEC_LZ4F and LZH_CODEC_NVLZ4; the nvcomp container has no ragged call.
 * What stays as 3b: d_in_ptrs, d_in_bytes, d_out_ptrs and d_out_bytes are device arrays of nchunks entries; chunk i is
 * the d_in_bytes[i] bytes at d_in_ptrs[i], any alignment; chunks may overlap or repeat; every input chunk needs 16
 * readable bytes after it; max_chunk_bytes at most 16 MiB, else LZH_EARG; nchunks == 0 returns LZH_OK and launches
 * nothing; a chunk whose device-side size passes max_chunk_bytes is not processed -- d_csizes[i] = 0 (it takes no
 * packed bytes) or d_status[i] = -1, and no kernel touches a slot for it; packed_cap is enforced on the device -- a
 * frame whose packed range would pass it is not written, d_csizes and d_offsets still report every size, and
 * d_offsets[nchunks] > packed_cap tells the caller that the output is incomplete; d_offsets of the decompress call may
 * be NULL (derived from d_csizes into d_temp); the raw-store rule holds on both sides, at frame level (a frame whose
 * size equals its chunk's is stored raw, and decoded as raw); every launch goes on hip_stream, with no side stream,
 * event, host synchronisation or size read back, so the calls can be captured in a stream.
 * Check order, all before any device call:
 *   1. level and max_chunk_bytes: LZH_EARG;
 *   2. nchunks == 0: LZH_OK;
 *   3. a null pointer (every pointer but hip_stream and the decompress call's d_offsets): LZH_EARG;
 *   4. the launch grid -- nchunks x the blocks per frame of max_chunk_bytes (compress: ceil(max_chunk_bytes / min(block
 *      size, max_chunk_bytes)), at least 1; decompress: ceil(max_chunk_bytes / 64 KiB), at least 1) must stay within
 *      0x7fffffff: LZH_EARG;
 *   5. temp_bytes below the sizing answer: LZH_ESPACE.
 * The three sizing functions are host arithmetic, non-decreasing in max_chunk_bytes and nchunks (total_in_bytes and
 * nchunks), and the two temp answers are 0 exactly where the calls return LZH_EARG for those arguments.
 * level: LZH_LZ4F_PARAMS(blockSizeID 0 | 4 .. 7, flags, acceleration), accepted exactly where
 * lzh_level_supported(LZH_CODEC_LZ4F, level, .) is 1 and LZH_LZ4F_LINKED is not set.  Linked-block compression is
 * not built here: with the flag the call returns LZH_EARG (the uniform call has the one-wave-per-frame linked kernel).
 * Compressed bytes: frame i is exactly what lzh_compress_async(LZH_CODEC_LZ4F, level, .., n = d_in_bytes[i],
 * chunk_size >= n) writes for that chunk alone, i.e. LZ4F_compressFrame with independent blocks: the header's
 * block-size id follows LZ4F_optimalBSID for the chunk's own size; content size, block checksums and content checksum
 * follow the flags; a block that LZ4 does not shrink is stored raw.  Equal sizes over contiguous input give the uniform
 * call's d_csizes, d_offsets and packed bytes.  A zero-length chunk is legal: the 11-byte frame (header, end mark), 15
 * bytes with a content checksum.  lzh_lz4f_ragged_max_packed_bytes is the capacity no batch of that total size and
 * chunk count exceeds.
 * Decoding: d_status[i] and the output bytes are those of lzh_decompress_async(LZH_CODEC_LZ4F, ..) for that frame and
 * n = chunk_size = d_out_bytes[i]: the decoded size, -1 malformed, -2 a feature outside the supported set (a frame
 * that does not decode to exactly d_out_bytes[i] bytes gets one of the two).  Independent and linked frames decode
 * alike.  An empty frame decodes to status 0 and writes nothing.  Output pointers of any alignment; nothing is written
 * past d_out_ptrs[i] + d_out_bytes[i].
 * Temp, compress: uniform slots.  With B the level's block size, bs = min(B, max_chunk_bytes) and bpf =
 * ceil(max_chunk_bytes / bs), every frame has bpf block slots; a block takes a staging slot, a sequence-record slot, a
 * record header, two u32 (its size, its offset in the frame) and 16 bytes of the block table (its pointer and size).  A
 * skewed batch therefore pays for its largest chunk nchunks times: 4096 chunks of which one has 16 MiB size as 4096
 * chunks of 16 MiB.  A compact layout is not built; the block table is what it would re-place (block slots from a scan
 * of per-chunk block counts).  Temp, decompress: scanned offsets, nchunks x ceil(max_chunk_bytes / 64 KiB) 32-byte
 * block descriptors and block statuses, nchunks frame statuses. */
size_t lzh_lz4f_ragged_compress_temp_bytes(int level, size_t max_chunk_bytes, size_t nchunks);
size_t lzh_lz4f_ragged_decompress_temp_bytes(size_t max_chunk_bytes, size_t nchunks);
size_t lzh_lz4f_ragged_max_packed_bytes(size_t total_in_bytes, size_t nchunks);
int lzh_lz4f_compress_ragged_async(int level, const void* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t nchunks,
                                   size_t max_chunk_bytes, void* d_packed, size_t packed_cap, uint32_t* d_csizes,
                                   uint64_t* d_offsets, void* d_temp, size_t temp_bytes, void* hip_stream);
int lzh_lz4f_decompress_ragged_async(const void* d_packed, size_t packed_readable, const uint32_t* d_csizes,
                                     const uint64_t* d_offsets, void* const* d_out_ptrs, const uint64_t* d_out_bytes,
                                     size_t nchunks, size_t max_chunk_bytes, int32_t* d_status, void* d_temp,
                                     size_t temp_bytes, void* hip_stream);

/* Dispatch the stages of lzh_compress_async separately (profiling / roofline): the codec
 * kernel alone writes the staging slots and per-chunk sizes. */
int lzh_compress_kernel_only(int codec, int level, const void* d_in, size_t n, size_t in_readable,
                             size_t chunk_size, void* d_stage, uint32_t* d_csizes, void* hip_stream);

/* One stage of lzh_compress_kernel_only (profiling, roofline of one kernel): stage_mask bit 0 =
 * the parse kernel (LZ4 / snappy: sequence records, chunks up to 16 MiB; zstd: the whole codec),
 * bit 1 = the LZ4 / snappy block-emission kernel (records -> staging slots and sizes).  Both
 * bits = lzh_compress_kernel_only. */
int lzh_compress_kernel_stage(int codec, int level, int stage_mask, const void* d_in, size_t n, size_t in_readable,
                              size_t chunk_size, void* d_stage, uint32_t* d_csizes, void* hip_stream);

/* The rest of lzh_compress_async after lzh_compress_kernel_only: scan the per-chunk sizes
 * into d_offsets and pack the staged streams (or the raw input) into d_packed. */
int lzh_compress_finish_async(int codec, const void* d_in, size_t n, size_t in_readable, size_t chunk_size,
                              const void* d_stage, const uint32_t* d_csizes, void* d_packed, size_t packed_cap,
                              uint64_t* d_offsets, void* hip_stream);

/* synthetic corpora of SURVEY.md 8(d): 0 random, 1 text, 2 json logs, 3 mixed, 4 binary */
size_t lzh_datagen(int kind, uint64_t seed, void* buf, size_t n);
const char* lzh_version(void);

#ifdef __cplusplus
}
#endif
#endif
