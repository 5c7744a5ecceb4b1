// lzbench_amd/csrc/zstd_dict_walk_main.cpp -- the host walk of zstd_dict_parse.h as a stand-alone program
// (`make dict_walk`, by default with -fsanitize=address,undefined): dictionaries and chunks of lzb_datagen's text and
// JSON corpora at the sizes of tests/zstd_dict_inputs.py, random bytes and zeros, levels 1 and -3; every walk's
// sequences are replayed over dictionary and chunk and must give the chunk back.  Buffers are allocated at their exact
// sizes plus the 16 readable bytes the interface asks for, so a read or write outside them is the sanitizer's to find.
// Exit status 0: every chunk rebuilt.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zstd_dict_parse.h"

extern "C" size_t lzb_datagen(int kind, uint64_t seed, uint8_t* buf, size_t n);

static bool replay(const std::vector<uint8_t>& d, size_t D, const std::vector<uint8_t>& c, size_t n,
                   const std::vector<uint32_t>& s, long k) {
    std::vector<uint8_t> out;
    out.reserve(n);
    uint32_t rep[3] = {1, 4, 8};
    for (long i = 0; i < k; i++) {
        const uint32_t ll = s[3 * i], ml = s[3 * i + 1], ob = s[3 * i + 2];
        if (out.size() + ll + ml > n) return false;
        out.insert(out.end(), c.begin() + out.size(), c.begin() + out.size() + ll);
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
    out.insert(out.end(), c.begin() + out.size(), c.begin() + n);
    return n == 0 || memcmp(out.data(), c.data(), n) == 0;
}

int main() {
    const size_t dicts[] = {8, 9, 11, 4095, 4096, 65536, 112640, 131072};
    const size_t sizes[] = {0, 1, 6, 7, 8, 9, 64, 300, 1000, 4099, 16384, 70000, 131072};
    const size_t bounds[] = {16384, 16385, 131072, 131073, 262144};
    const int levels[] = {1, -3};
    std::vector<uint32_t> tab(1u << 15);
    long walks = 0, seqs = 0;
    for (int kind = 1; kind <= 2; kind++) {              // 1 text, 2 JSON
        std::vector<uint8_t> stream(131072 + 400000);
        lzb_datagen(kind, 50 + (uint64_t)kind, stream.data(), stream.size());
        for (size_t D : dicts) {
            std::vector<uint8_t> d(D + 16);
            memcpy(d.data(), stream.data() + 131072 - D, D);
            std::vector<size_t> ns(sizes, sizes + sizeof sizes / sizeof *sizes);
            for (size_t t : bounds)
                if (t > D && t - D <= 131072) ns.push_back(t - D);
            for (size_t n : ns) {
                for (int fill = 0; fill < 3; fill++) {   // the corpus, random bytes, zeros
                    std::vector<uint8_t> c(n + 16);
                    if (fill == 0) memcpy(c.data(), stream.data() + 131072 + (n * 7) % 200000, n);
                    else if (fill == 1) lzb_datagen(0, 100 + n % 89, c.data(), n);
                    for (int level : levels) {
                        std::vector<uint32_t> s(3 * (n / 4 + 16));
                        const long k = zdd::host_walk(level, d.data(), D, c.data(), n, s.data(), n / 4 + 16, tab.data());
                        if (k < 0 || (size_t)k > n / 4 + 16 || !replay(d, D, c, n, s, k)) {
                            fprintf(stderr, "kind %d dict %zu chunk %zu fill %d level %d: walk %ld does not rebuild the chunk\n",
                                    kind, D, n, fill, level, k);
                            return 1;
                        }
                        walks++;
                        seqs += k;
                    }
                }
            }
        }
    }
    printf("zstd dictionary walk: %ld walks, %ld sequences, every chunk rebuilt\n", walks, seqs);
    return 0;
}
