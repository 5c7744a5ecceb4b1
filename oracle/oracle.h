/*
 * oracle/oracle.h -- CPU restatement of the reference codecs on the lzbench hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product (lzbench_amd/, include/, the
 * C-ABI library) may include, link or call anything under oracle/.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg use it, and only as the
 * checker / CPU baseline, never as the thing measured on the GPU.
 *
 * Pinning: these restatements are checked byte-for-byte against golden vectors
 * produced by the reference's own lz4 1.9.3 / snappy 1.1.8 sources compiled from
 * /root/reference (oracle/Makefile target `ref`, outputs in oracle/_ref/), see
 * tests/golden/make_golden.py and tests/test_oracle.py.
 */
#ifndef LZB_ORACLE_H
#define LZB_ORACLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* LZ4 block compression, LZ4_compress_fast(src,dst,n,cap>=bound,acc) semantics
 * (reference lz4/lz4.c:1284-1305 notLimited path, :851-1240 parser). Returns bytes written. */
int oracle_lz4_compress(const uint8_t* src, int n, uint8_t* dst, int acceleration);
/* The same compressor, counting its parser's events into c[ORACLE_LZ4C_N] (added to what c holds; the bytes
 * written are oracle_lz4_compress's: one body).  tests/lzc_census.py names and documents the events. */
enum {
    ORACLE_LZ4C_TAB_U16, ORACLE_LZ4C_TAB_U32, ORACLE_LZ4C_N_LT_13,
    ORACLE_LZ4C_HIT_SEARCH, ORACLE_LZ4C_HIT_RETEST, ORACLE_LZ4C_RETEST_CHAIN_8,
    ORACLE_LZ4C_CATCHUP_0, ORACLE_LZ4C_CATCHUP_1_3, ORACLE_LZ4C_CATCHUP_4, ORACLE_LZ4C_CATCHUP_5_64,
    ORACLE_LZ4C_CATCHUP_GT_64, ORACLE_LZ4C_CATCHUP_TO_ANCHOR, ORACLE_LZ4C_CATCHUP_TO_START,
    ORACLE_LZ4C_COUNT_0, ORACLE_LZ4C_COUNT_1_19, ORACLE_LZ4C_COUNT_20, ORACLE_LZ4C_COUNT_21_275,
    ORACLE_LZ4C_COUNT_GT_275, ORACLE_LZ4C_COUNT_GT_262164, ORACLE_LZ4C_COUNT_TO_MATCHLIMIT,
    ORACLE_LZ4C_LIT_0, ORACLE_LZ4C_LIT_1_14, ORACLE_LZ4C_LIT_15, ORACLE_LZ4C_LIT_16_255, ORACLE_LZ4C_LIT_256UP,
    ORACLE_LZ4C_LIT_270, ORACLE_LZ4C_ML_15, ORACLE_LZ4C_ML_15_255,
    ORACLE_LZ4C_OFF_1, ORACLE_LZ4C_OFF_2_3, ORACLE_LZ4C_OFF_65535, ORACLE_LZ4C_FAR_REJECTED, ORACLE_LZ4C_FAR_65536,
    ORACLE_LZ4C_STEP_GT_1, ORACLE_LZ4C_STEP_GT_ACC,
    ORACLE_LZ4C_END_SEARCH, ORACLE_LZ4C_END_MATCH, ORACLE_LZ4C_LAST_LITERALS_5, ORACLE_LZ4C_SEQUENCES,
    ORACLE_LZ4C_N
};
int oracle_lz4_compress_census(const uint8_t* src, int n, uint8_t* dst, int acceleration, uint64_t* c);
/* LZ4_compressBound (reference lz4/lz4.h:171). */
int oracle_lz4_bound(int n);
/* LZ4_decompress_safe semantics (reference lz4/lz4.c:1737-2165 safe loop, :2170-2176).
 * Returns decoded size, or a negative value on malformed input. */
int oracle_lz4_decompress_safe(const uint8_t* src, int csize, uint8_t* dst, int cap);
int oracle_lz4_decompress_prefix(const uint8_t* src, int csize, uint8_t* dst, int cap, int64_t prefix);

/* snappy::RawCompress (reference snappy/snappy.cc:1043-1111, :510-681). Returns bytes written. */
size_t oracle_snappy_compress(const uint8_t* src, size_t n, uint8_t* dst);
/* The same compressor, counting its parser's events into c[ORACLE_SNC_N] (added to what c holds; one body).
 * TABLE_256 + k: a fragment with a table of 256 << k entries (k = 0..6).  tests/lzc_census.py names the events. */
enum {
    ORACLE_SNC_TABLE_256, ORACLE_SNC_TABLE_512, ORACLE_SNC_TABLE_1024, ORACLE_SNC_TABLE_2048, ORACLE_SNC_TABLE_4096,
    ORACLE_SNC_TABLE_8192, ORACLE_SNC_TABLE_16384,
    ORACLE_SNC_FRAG_LT_15, ORACLE_SNC_FRAGS_1, ORACLE_SNC_FRAGS_2, ORACLE_SNC_FRAGS_4UP,
    ORACLE_SNC_HIT_SEARCH, ORACLE_SNC_HIT_RETEST, ORACLE_SNC_PROBE_PAST_16, ORACLE_SNC_PROBE_OFF_GT_63,
    ORACLE_SNC_SEARCH_RAN_OUT, ORACLE_SNC_END_COPY,
    ORACLE_SNC_COPY1, ORACLE_SNC_COPY2_LEN, ORACLE_SNC_COPY2_OFF,
    ORACLE_SNC_COPY_64, ORACLE_SNC_COPY_65_67, ORACLE_SNC_COPY_68, ORACLE_SNC_COPY_132UP,
    ORACLE_SNC_LIT_1_60, ORACLE_SNC_LIT_61_256, ORACLE_SNC_LIT_257_65536, ORACLE_SNC_LIT_GT_256_BEFORE_COPY,
    ORACLE_SNC_LIT_REMAINDER,
    ORACLE_SNC_N
};
size_t oracle_snappy_compress_census(const uint8_t* src, size_t n, uint8_t* dst, uint64_t* c);
/* snappy::MaxCompressedLength (reference snappy/snappy.cc:99-121). */
size_t oracle_snappy_bound(size_t n);
/* snappy::RawUncompress (reference snappy/snappy.cc:848-1036, :1398-1407).
 * Returns the uncompressed size on success, -1 on malformed input. cap = output capacity. */
int64_t oracle_snappy_uncompress(const uint8_t* src, size_t csize, uint8_t* dst, size_t cap);

/* zstd 1.5.2 frame compression as lzbench's zstd rows call it (ZSTD_getParams(level, n, 0) with
 * contentSizeFlag, ZSTD_compress_advanced; reference _lzbench/compressors.cpp:1745-1770), for the
 * fast-strategy levels (-131072..-1, 1, 2; level 2 only where it is fast).  dst needs
 * oracle_zstd_bound(n) + 64 bytes.  Returns the frame size, or -1 for an unsupported level. */
int64_t oracle_zstd_compress(const uint8_t* src, size_t n, uint8_t* dst, int level);
size_t oracle_zstd_bound(size_t n);
/* The same compressor, counting the decisions of its entropy stage into c[ORACLE_ZSE_N] (added to what c holds; the
 * bytes written are oracle_zstd_compress's: one body; c == NULL counts nothing).  tests/zstd_entropy_census.py names
 * and documents the events, in this order.  The FSE events (NORM_FAST .. NC_FLUSH_MID_RUN) exist once per call site:
 * index + ORACLE_ZSE_FSE_STRIDE * site, site 0 = the sequence tables, 1 = the Huffman weights.  The per-table events
 * (TYPE_RLE .. TLOG_9) exist three times: index + ORACLE_ZSE_TAB_STRIDE * table, table 0 = LL, 1 = OF, 2 = ML. */
enum {
    ORACLE_ZSE_LIT_GATE_LE63, ORACLE_ZSE_LIT_GATE_63, ORACLE_ZSE_LIT_GATE_64, ORACLE_ZSE_LIT_OFF,
    ORACLE_ZSE_LIT_SAMPLED_RAW, ORACLE_ZSE_LIT_SAMPLED_PASSED, ORACLE_ZSE_LIT_SUSPECT_19, ORACLE_ZSE_LIT_SUSPECT_20,
    ORACLE_ZSE_LIT_RLE, ORACLE_ZSE_LIT_FLAT_RAW, ORACLE_ZSE_LIT_REPEAT_INVALID, ORACLE_ZSE_LIT_REPEAT_SMALL_DIRECT,
    ORACLE_ZSE_LIT_REPEAT_OLD_BY_ESTIMATE, ORACLE_ZSE_LIT_REPEAT_OLD_BY_H12, ORACLE_ZSE_LIT_REPEAT_NEW_TABLE,
    ORACLE_ZSE_LIT_RAW_H12, ORACLE_ZSE_LIT_RAW_STREAMS_OLD, ORACLE_ZSE_LIT_RAW_STREAMS_NEW, ORACLE_ZSE_LIT_RAW_MINGAIN,
    ORACLE_ZSE_LIT_HDR_3, ORACLE_ZSE_LIT_HDR_4, ORACLE_ZSE_LIT_HDR_5, ORACLE_ZSE_LIT_STREAMS_1, ORACLE_ZSE_LIT_STREAMS_4,
    ORACLE_ZSE_LIT_STREAM_GT_65535,
    ORACLE_ZSE_HUF_MAXNB_5, ORACLE_ZSE_HUF_MAXNB_6, ORACLE_ZSE_HUF_MAXNB_7, ORACLE_ZSE_HUF_MAXNB_8, ORACLE_ZSE_HUF_MAXNB_9,
    ORACLE_ZSE_HUF_MAXNB_10, ORACLE_ZSE_HUF_MAXNB_11, ORACLE_ZSE_HUF_MAXNB_BY_MAX11, ORACLE_ZSE_HUF_MAXNB_BY_SRCSIZE,
    ORACLE_ZSE_HUF_MAXNB_BY_MINBITS, ORACLE_ZSE_HUF_MAXNB_BY_FLOOR5,
    ORACLE_ZSE_HUF_LIMIT_NOT_NEEDED, ORACLE_ZSE_HUF_LIMIT_FIRED, ORACLE_ZSE_HUF_LIMIT_REPAY_DEC_GT1,
    ORACLE_ZSE_HUF_LIMIT_REPAY_NO_SYMBOL, ORACLE_ZSE_HUF_LIMIT_OVERPAID, ORACLE_ZSE_HUF_LIMIT_OVERPAID_RANK1_EMPTY,
    ORACLE_ZSE_HUF_SORT_BUCKET_GE165, ORACLE_ZSE_HUF_SORT_PARTITIONED,
    ORACLE_ZSE_HUF_W_WN_LE1, ORACLE_ZSE_HUF_W_RLE, ORACLE_ZSE_HUF_W_ALL_DISTINCT, ORACLE_ZSE_HUF_W_FSE,
    ORACLE_ZSE_HUF_W_FSE_TOO_LARGE, ORACLE_ZSE_HUF_W_ODD_COUNT,
    ORACLE_ZSE_HUF_TABLE_DIRECT, ORACLE_ZSE_HUF_TABLE_FSE, ORACLE_ZSE_HUF_TABLE_REFUSED,
    ORACLE_ZSE_M2_TODIST_0, ORACLE_ZSE_M2_SECOND_PASS, ORACLE_ZSE_M2_ALL_LOW, ORACLE_ZSE_M2_TOTAL_0, ORACLE_ZSE_M2_SPREAD,
    ORACLE_ZSE_SEQ_NS_MOD64_0, ORACLE_ZSE_SEQ_NS_MOD64_1, ORACLE_ZSE_SEQ_NS_MOD64_2, ORACLE_ZSE_SEQ_NS_MOD64_3,
    ORACLE_ZSE_SEQ_NS_MOD64_4, ORACLE_ZSE_SEQ_NS_MOD64_5,
    ORACLE_ZSE_SEQ_NS_1, ORACLE_ZSE_SEQ_NS_63, ORACLE_ZSE_SEQ_NS_64, ORACLE_ZSE_SEQ_NS_65, ORACLE_ZSE_SEQ_NS_128,
    ORACLE_ZSE_SEQ_NS_129,
    ORACLE_ZSE_SEQ_BITS_GE32, ORACLE_ZSE_SEQ_BITS_GE57, ORACLE_ZSE_SEQ_LL_GE65536, ORACLE_ZSE_SEQ_ML_GE65539,
    ORACLE_ZSE_SEQ_OFCODE_GE17,
    ORACLE_ZSE_BLOCK_LEN_LT7, ORACLE_ZSE_BLOCK_RAW_MINGAIN, ORACLE_ZSE_BLOCK_RAW_SEQUENCES_FAILED, ORACLE_ZSE_BLOCK_RLE,
    ORACLE_ZSE_BLOCK_RLE_REFUSED_FIRST, ORACLE_ZSE_BLOCK_CMP_NEW_HUF_KEPT, ORACLE_ZSE_BLOCK_REPCODES_CONFIRMED,
    ORACLE_ZSE_BLOCK_REPCODES_UNCONFIRMED,
    ORACLE_ZSE_FSE0,                                       /* first FSE event of site 0 */
    ORACLE_ZSE_NORM_FAST = ORACLE_ZSE_FSE0, ORACLE_ZSE_NORM_P_LT8_ROUNDED_UP, ORACLE_ZSE_NORM_LOW_MINUS1,
    ORACLE_ZSE_NORM_LOW_PLUS1, ORACLE_ZSE_NORM_M2,
    ORACLE_ZSE_NC_ZERO_RUN_0, ORACLE_ZSE_NC_ZERO_RUN_1_2, ORACLE_ZSE_NC_ZERO_RUN_3UP, ORACLE_ZSE_NC_ZERO_RUN_24UP,
    ORACLE_ZSE_NC_COUNT_GE_THRESHOLD, ORACLE_ZSE_NC_ENDS_EARLY, ORACLE_ZSE_NC_FLUSH_MID_RUN,
    ORACLE_ZSE_FSE_STRIDE = ORACLE_ZSE_NC_FLUSH_MID_RUN + 1 - ORACLE_ZSE_FSE0,
    ORACLE_ZSE_TAB0 = ORACLE_ZSE_FSE0 + 2 * ORACLE_ZSE_FSE_STRIDE,     /* first per-table event of LL */
    ORACLE_ZSE_TYPE_RLE = ORACLE_ZSE_TAB0, ORACLE_ZSE_TYPE_RLE_AS_PREDEF, ORACLE_ZSE_TYPE_PREDEF_BY_COUNT,
    ORACLE_ZSE_TYPE_PREDEF_BY_FLATNESS, ORACLE_ZSE_TYPE_FSE, ORACLE_ZSE_TYPE_DEFAULT_REFUSED,
    ORACLE_ZSE_LAST_COUNT_TAKEN, ORACLE_ZSE_LAST_COUNT_NOT,
    ORACLE_ZSE_TLOG_5, ORACLE_ZSE_TLOG_6, ORACLE_ZSE_TLOG_7, ORACLE_ZSE_TLOG_8, ORACLE_ZSE_TLOG_9,
    ORACLE_ZSE_TAB_STRIDE = ORACLE_ZSE_TLOG_9 + 1 - ORACLE_ZSE_TAB0,
    ORACLE_ZSE_N = ORACLE_ZSE_TAB0 + 3 * ORACLE_ZSE_TAB_STRIDE
};
int64_t oracle_zstd_compress_census(const uint8_t* src, size_t n, uint8_t* dst, int level, uint64_t* c);

/* Framed LZ4 formats (frame_oracle.c).  LZ4 frame as LZ4F_compressFrame writes it with
 * independent blocks (lz4frame.c:373-1019); params: bits 0-2 blockSizeID (0 = default 64 KiB, 4..7),
 * 0x10 block checksum, 0x20 content checksum, 0x40 content size, bits 8-15 acceleration.
 * nvcomp LZ4 container (nvcomp/LZ4Metadata.h): chunks of 1 << (15 + level) bytes, LZ4 blocks.
 * Decoders return the decoded size, -1 on malformed input, -2 for an unsupported feature. */
uint32_t oracle_xxh32(const uint8_t* p, size_t len, uint32_t seed);
size_t  oracle_lz4f_bound(size_t n, int params);
int64_t oracle_lz4f_compress(const uint8_t* src, size_t n, uint8_t* dst, int params);
int64_t oracle_lz4f_decompress(const uint8_t* src, size_t csize, uint8_t* dst, size_t cap);
size_t  oracle_nvlz4_bound(size_t n, int level);
int64_t oracle_nvlz4_compress(const uint8_t* src, size_t n, uint8_t* dst, int level);
int64_t oracle_nvlz4_decompress(const uint8_t* src, size_t csize, uint8_t* dst, size_t cap);

/* lzbench chunk loop (reference _lzbench/lzbench.cpp:266-298): compress every chunk,
 * store raw when clen<=0 || clen==part, pack contiguously. codec: 0=lz4 1=snappy 2=zstd
 * (compression only) 3=lz4 frame 4=nvcomp lz4 container (level = their params).
 * level: lz4 acceleration (0 or 1 -> default). Returns total packed bytes. */
int64_t oracle_compress_chunks(int codec, int level, const uint8_t* in, size_t n,
                               size_t chunk_size, uint8_t* out, uint64_t* csizes);
/* lzbench_decompress (reference _lzbench/lzbench.cpp:301-329). Returns total or <=0 on error. */
int64_t oracle_decompress_chunks(int codec, const uint8_t* packed, const uint64_t* csizes,
                                 size_t n, size_t chunk_size, uint8_t* out);
/* Same loops over the chunk list split across `threads` pthreads (CPU baseline, all cores). */
int64_t oracle_compress_chunks_mt(int codec, int level, const uint8_t* in, size_t n,
                                  size_t chunk_size, uint8_t* out, uint64_t* csizes, int threads);
int64_t oracle_decompress_chunks_mt(int codec, const uint8_t* packed, const uint64_t* csizes,
                                    size_t n, size_t chunk_size, uint8_t* out, int threads);

#ifdef __cplusplus
}
#endif
#endif
