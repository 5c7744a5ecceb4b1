// lzbench_amd/csrc/zstdd_exec_body.inc -- body of the zstd split decoder's execution kernels (lzh_zstd_exec_kernel,
// decode_hip.hip; lzh_zstd_exec_ragged_kernel, zstd_ragged_split_hip.hip) for a frame the header and literal
// kernels left at kGo.  The including kernel has: win (its LDS), lane, chunk, out + ooff, n_total, chunk_size (as in
// zstdd_hdr_body.inc), packed, packed_readable, offsets, csizes, status, zt, zst, zfr.
// A third consumer, lzh_zstd_exec_compact_kernel (zstd_ragged_split_compact_hip.hip), passes the frame's own size as
// chunk_size and a zsplit::Placed as zt: as in zstdd_hdr_body.inc, keep the area `zt + chunk * Z.stride`.
// Textual, not a function: see zstdd_hdr_body.inc.
    const int sv = zfr[chunk].sv;                                // then the sequence kernel's
    if (sv != zsplit::kGo) {
        if (lane == 0) {
            if (sv == zsplit::kLegacy) {
                zst[chunk] = zsplit::kLegacy;
            } else {
                status[chunk] = sv;
                zst[chunk] = zsplit::kDone;
            }
        }
        return;
    }
    const int part = (int)min(chunk_size, n_total - ooff);
    const uint64_t ioff = offsets[chunk];
    const int cs = (int)csizes[chunk];
    const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, (uint64_t)cs + 16) : 0;
    Bytes rin, rout, lout;
    rin.init(packed + ioff, readable);
    rout.init(out + ooff, (uint64_t)part);
    lout.init(out + ooff, (uint64_t)part + 3);
    const zsplit::ZLayout Z = zsplit::zlayout(chunk_size);
    zstdd::ZSink O{(LDSA uint8_t*)win, rout, 0, 0};
    const int r = zsplit::exec_frame(rin, rout, lout, O, (LDSA uint8_t*)win + zstdd::kZW, zt + chunk * Z.stride, Z,
                                     zfr[chunk], lane);
    if (lane == 0) status[chunk] = r;
