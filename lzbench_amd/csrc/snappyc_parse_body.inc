// lzbench_amd/csrc/snappyc_parse_body.inc -- body of the snappy parse kernels (lzh_snappy_parse_kernel,
// snappyc_hip.hip; lzh_snappy_parse_ragged_kernel, ragged_hip.hip) after the chunk lookup.  The including kernel
// has: chunk (its index), f (the fragment), in + off (the chunk's address), in_readable - off (bytes that may be
// read from there), n (its size), lds, recs, rec_stride, rec_hdr, frags.  Textual, not a function: the uniform
// kernel's code must stay bit-identical (its traffic profile is keyed to its code hash) and the compiler lays a
// hoisted body out differently.
    const rsrc_t rr = make_rsrc(recs + chunk * rec_stride, (uint32_t)rec_stride);
    uint32_t* hdr = rec_hdr + chunk * frags;       // end record (exclusive) of each fragment
    int nrec = frags > 1 ? (int)f * kFragRecs : 0;
    const uint32_t fpos = f << 16;
    if (fpos < n) {
        const int fn = (int)min(65536u, n - fpos);
        const uint64_t readable = min<uint64_t>(in_readable - off - fpos, (uint64_t)fn + 64);
        Bytes rin, rout;
        rin.init(in + off + fpos, readable);
        rout.init(nullptr, 0);
        snv2::compress_fragment<true>(rin, fn, rout, 0, (LDSA uint16_t*)lds, (LDSA uint32_t*)lds + (1 << 13), nullptr,
                                      nullptr, rr, nrec, (int)fpos);
    }
    if (threadIdx.x == 0) hdr[f] = (uint32_t)nrec;
