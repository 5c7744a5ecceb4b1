// lzbench_amd/csrc/zstd_dfast_dict_walk_main.cpp -- the host walk of zstd_dfast_dict_parse.h as a stand-alone program
// (`make dfast_dict_walk`, by default with -fsanitize=address,undefined) over (dictionary, chunk) pairs read from a
// file: records of two little-endian u32 (dictionary bytes, chunk bytes) followed by the dictionary and the chunk
// (tests/test_zstd_dfast_dict_walk.py writes the constructed pairs of tests/zstd_dfast_dict_inputs.py).  Without a
// file: three pairs made here.  Every buffer is allocated at its exact size plus the 16 readable bytes the interface
// asks for, so a read or write outside them is the sanitizer's to find; every walk's sequences are replayed over
// dictionary and chunk and must give the chunk back.  One line per pair: its sizes, sequences and event counters.
// Exit status 0: every chunk rebuilt.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zstd_dfast_dict_parse.h"

static bool replay(const uint8_t* d, size_t D, const uint8_t* c, size_t n, const uint32_t* s, long k) {
    std::vector<uint8_t> out;
    out.reserve(n);
    uint32_t rep[3] = {1, 4, 8};
    for (long i = 0; i < k; i++) {
        const uint32_t ll = s[3 * i], ml = s[3 * i + 1], ob = s[3 * i + 2];
        if (out.size() + ll + ml > n) return false;
        out.insert(out.end(), c + out.size(), c + out.size() + ll);
        uint32_t off;
        if (ob > 3) {
            off = ob - 3;
            rep[2] = rep[1]; rep[1] = rep[0]; rep[0] = off;
        } else {
            if (ob != 1) return false;
            if (ll == 0) { const uint32_t t = rep[0]; rep[0] = rep[1]; rep[1] = t; }
            off = rep[0];
        }
        if (off > out.size() + D) return false;
        for (uint32_t j = 0; j < ml; j++) {
            const long p = (long)out.size() - (long)off;
            out.push_back(p < 0 ? d[D + p] : out[(size_t)p]);
        }
    }
    out.insert(out.end(), c + out.size(), c + n);
    return n == 0 || memcmp(out.data(), c, n) == 0;
}

// one pair, both buffers copied into exact-size heap blocks
static bool one(const uint8_t* dict, size_t D, const uint8_t* chunk, size_t n, std::vector<uint32_t>& tab) {
    uint8_t* d = (uint8_t*)malloc(D + 16);
    uint8_t* c = (uint8_t*)malloc(n + 16);
    uint32_t* s = (uint32_t*)malloc(3 * (n / 4 + 16) * sizeof(uint32_t));
    memcpy(d, dict, D);
    memset(d + D, 0, 16);
    memcpy(c, chunk, n);
    memset(c + n, 0, 16);
    uint64_t ev[zfd::kEvents] = {};
    const long k = zfd::host_walk(3, d, D, c, n, s, n / 4 + 16, tab.data(), ev);
    const bool ok = k >= 0 && (size_t)k <= n / 4 + 16 && replay(d, D, c, n, s, k);
    printf("dict %zu chunk %zu: %ld sequences%s; events", D, n, k, ok ? "" : " DO NOT REBUILD THE CHUNK");
    for (int i = 0; i < zfd::kEvents; i++) printf(" %llu", (unsigned long long)ev[i]);
    printf("\n");
    free(s);
    free(c);
    free(d);
    return ok;
}

int main(int argc, char** argv) {
    std::vector<uint32_t> tab(2u << 16);
    long pairs = 0;
    bool ok = true;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
        uint32_t h[2];
        while (fread(h, 4, 2, f) == 2) {
            if (h[0] < zfd::kDictMin || h[0] > zfd::kDictMax || h[1] > zfd::kChunkMax) { fprintf(stderr, "bad record\n"); return 2; }
            std::vector<uint8_t> d(h[0]), c(h[1]);
            if (fread(d.data(), 1, h[0], f) != h[0] || fread(c.data(), 1, h[1], f) != h[1]) { fprintf(stderr, "short record\n"); return 2; }
            ok &= one(d.data(), h[0], c.data(), h[1], tab);
            pairs++;
        }
        fclose(f);
    } else {
        // a dictionary of a short period, and chunks that repeat it, cross its end and are it
        std::vector<uint8_t> d(4096), c(6000);
        uint32_t x = 12345;
        for (size_t i = 0; i < d.size(); i++) { x = x * 1103515245u + 12345u; d[i] = (uint8_t)(i % 700 < 650 ? (i % 700) * 7 : x >> 24); }
        for (size_t i = 0; i < c.size(); i++) { x = x * 1103515245u + 12345u; c[i] = (uint8_t)(i % 900 < 800 ? d[(i * 3) % 4000 + (i % 50)] : x >> 24); }
        ok &= one(d.data(), d.size(), c.data(), c.size(), tab);
        ok &= one(d.data(), d.size(), d.data(), d.size(), tab);
        ok &= one(d.data(), 8, c.data(), 300, tab);
        pairs = 3;
    }
    printf("zstd level-3 dictionary walk: %ld pairs, %s\n", pairs, ok ? "every chunk rebuilt" : "FAILED");
    return ok && pairs ? 0 : 1;
}
