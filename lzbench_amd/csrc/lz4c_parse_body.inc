// lzbench_amd/csrc/lz4c_parse_body.inc -- body of the LZ4 parse kernels (lzh_lz4_parse_kernel, lz4c_hip.hip;
// lzh_lz4_parse_ragged_kernel, ragged_hip.hip) after the chunk lookup.  The including kernel has: chunk (its
// index), in + off (its address), readable (bytes that may be read from there), n (its size), lds, acc, recs,
// rec_stride, rec_hdr.  Textual, not a function: the uniform kernel's code must stay bit-identical (its traffic
// profile is keyed to its code hash) and the compiler lays a hoisted body out differently.
    Bytes rin, rout;
    rin.init(in + off, readable);
    rout.init(nullptr, 0);
    LDSA uint32_t* tab = (LDSA uint32_t*)lds;
    LDSA uint32_t* ring = tab + 4096;
    const rsrc_t rr = make_rsrc(recs + chunk * rec_stride, (uint32_t)rec_stride);
    uint32_t* hdr = rec_hdr + 2 * chunk;
    if (n < 65547) {
        if (acc > 1) lz4v3::compress_chunk<true, false, true, true>(rin, n, rout, acc, tab, ring, nullptr, nullptr, nullptr, rr, hdr);
        else lz4v3::compress_chunk<true, false, true, false>(rin, n, rout, acc, tab, ring, nullptr, nullptr, nullptr, rr, hdr);
    } else {
        if (acc > 1) lz4v3::compress_chunk<false, false, true, true>(rin, n, rout, acc, tab, ring, nullptr, nullptr, nullptr, rr, hdr);
        else lz4v3::compress_chunk<false, false, true, false>(rin, n, rout, acc, tab, ring, nullptr, nullptr, nullptr, rr, hdr);
    }
