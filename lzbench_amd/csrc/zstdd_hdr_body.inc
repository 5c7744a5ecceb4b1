// lzbench_amd/csrc/zstdd_hdr_body.inc -- body of the zstd split decoder's header kernels (lzh_zstd_hdr_kernel,
// decode_hip.hip; lzh_zstd_hdr_ragged_kernel, zstd_ragged_split_hip.hip) after the frame lookup.  The including
// kernel has: L (its LDS), lane, chunk (the frame's index: its temp slot, its entries of offsets / csizes / status /
// zst / zfr), out + ooff (the frame's output address), min(chunk_size, n_total - ooff) (its size), chunk_size (the
// largest frame of the launch: the per-frame temp is laid out for it), packed, packed_readable, offsets, csizes,
// status, zt, zst, zfr, stats, jobs, njobs.
// A third consumer, lzh_zstd_hdr_compact_kernel (zstd_ragged_split_compact_hip.hip), passes the frame's own size as
// chunk_size and a zsplit::Placed as zt, whose operator+ drops what is added: the body must keep naming the frame's
// area `zt + chunk * Z.stride`, zt first and one sum, or that kernel addresses another frame's area.
// Textual, not a function: the uniform kernel's code must stay bit-identical (profiles are keyed to kernel code
// hashes).
    const int part = (int)min(chunk_size, n_total - ooff);
    const uint64_t ioff = offsets[chunk];
    const int cs = (int)csizes[chunk];
    const uint64_t readable = ioff < packed_readable ? min<uint64_t>(packed_readable - ioff, (uint64_t)cs + 16) : 0;
    Bytes rin, rout;
    rin.init(packed + ioff, readable);
    rout.init(out + ooff, (uint64_t)part);
    if (cs == part) {                                  // stored raw by the chunk loop (lzbench.cpp:284-288)
        copy_raw(rin, rout, part, lane);
        if (lane == 0) {
            status[chunk] = part;
            zst[chunk] = zsplit::kDone;
        }
        return;
    }
    const zsplit::ZLayout Z = zsplit::zlayout(chunk_size);
    zsplit::ZFrame fr{0, 0, -1, 0, 0, 0, 0, 0};
    const int r = zsplit::hdr_frame(rin, rout, cs, L, part, zt + chunk * Z.stride, Z, fr, lane, stats, jobs, njobs,
                                    (uint32_t)chunk);
    if (lane == 0) {
        if (r == zsplit::kGo) zfr[chunk] = fr;
        zst[chunk] = r == zsplit::kGo ? zsplit::kGo : (r == zsplit::kLegacy ? zsplit::kLegacy : zsplit::kDone);
        if (r < 0) status[chunk] = r;
    }
