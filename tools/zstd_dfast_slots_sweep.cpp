// tools/zstd_dfast_slots_sweep.cpp -- the placement sweep of lzbench_amd/csrc/zstd_dfast_slots.h as a stand-alone host
// program, for a sanitizer build (the header is plain C++ on the host; nothing here touches a device):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
//       -I$ROCM/include tools/zstd_dfast_slots_sweep.cpp -o /tmp/zstd_dfast_slots_sweep && /tmp/zstd_dfast_slots_sweep
// For seeded lists of chunk sizes (the boundary sizes of ZSTD_getParams, random sizes, one 16 MiB chunk) it places
// every chunk by the exclusive scans of the slot sizes, as the device does, and checks that a batch that keeps its
// promise fits the two regions, that the regions never pass nchunks x the worst slot, that the worst slot bounds
// every slot, and that the region sizes are non-decreasing in each argument.  Exit status 0: all held.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../lzbench_amd/csrc/zstd_dfast_slots.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: %s failed (seed %d)\n", __FILE__, __LINE__, #c, seed); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main() {
    const uint64_t kMax = 16ull << 20;
    const uint64_t pool[] = {0, 1, 63, 64, 65, 16384, 16385, 131072, 131073, 262144, 262145};
    const uint64_t tops[] = {70, 5000, 20000, 140000, 300000};
    size_t placed = 0;
    int seed = 0;
    for (seed = 0; seed < 2000; seed++) {
        std::mt19937_64 rng(seed);
        const size_t k = 1 + rng() % 64;
        const uint64_t top = tops[rng() % 5];
        std::vector<uint64_t> sizes(k);
        for (auto& s : sizes) s = rng() % 2 ? pool[rng() % 11] : rng() % (top + 1);
        if (seed % 5 == 0) sizes[rng() % k] = kMax;
        uint64_t total = 0, maxb = 0;
        for (uint64_t s : sizes) { total += s; maxb = s > maxb ? s : maxb; }
        const LzhCompactRegions reg = lzh_zdslot_regions(total, maxb, k);
        CHECK(reg.stage % 256 == 0 && reg.recs % 256 == 0);
        CHECK(reg.stage <= k * lzh_zdslot_stage_bytes(maxb) && reg.recs <= k * lzh_zdslot_scratch_worst(maxb));
        std::vector<uint8_t> stage_map(reg.stage / 256, 0), scratch_map(reg.recs / 256, 0);   // one flag per 256 bytes
        uint64_t so = 0, ro = 0;
        for (uint64_t n : sizes) {
            const uint64_t ss = lzh_zdslot_stage_bytes(n), rs = lzh_zdslot_scratch_bytes(n);
            const LzhZdLayout lo = lzh_zdslot_layout(lzh_zdslot_params(n));
            const zdf::DParams P = lzh_zdslot_params(n);
            CHECK(ss % 256 == 0 && rs % 256 == 0 && rs == lo.stride);
            CHECK(rs <= lzh_zdslot_scratch_worst(maxb) && ss <= lzh_zdslot_stage_bytes(maxb));
            // what the kernel bodies address inside the slot: each area ends where the next starts or before
            CHECK(lo.seq_off == 1024 && lo.lit_off - lo.seq_off >= ((uint64_t)P.bsize / 4 + 16) * 8);
            CHECK(lo.att_off - lo.lit_off >= (uint64_t)P.bsize + 64 && lo.tab_off - lo.tmp_off >= (uint64_t)P.bsize + 256);
            CHECK(lo.tab_off + (4ull << P.hlog) + (4ull << P.clog) <= lo.stride);
            CHECK(so + ss <= reg.stage && ro + rs <= reg.recs);
            for (uint64_t b = so / 256; b < (so + ss) / 256; b++) { CHECK(!stage_map[b]); stage_map[b] = 1; }
            for (uint64_t b = ro / 256; b < (ro + rs) / 256; b++) { CHECK(!scratch_map[b]); scratch_map[b] = 1; }
            so += ss;
            ro += rs;
            placed++;
        }
        // non-decreasing in each argument
        const LzhCompactRegions a = lzh_zdslot_regions(total + 1 + rng() % 100000, maxb, k),
                                b = lzh_zdslot_regions(total, maxb + 1 + rng() % 100000, k),
                                c = lzh_zdslot_regions(total, maxb, k + 1 + rng() % 100);
        CHECK(a.stage >= reg.stage && a.recs >= reg.recs && b.stage >= reg.stage && b.recs >= reg.recs);
        CHECK(c.stage >= reg.stage && c.recs >= reg.recs);
    }
    // the worst slot bounds the slot of every size up to it, size by size over the small classes
    seed = -1;
    uint64_t worst_seen = 0;
    for (uint64_t n = 0; n <= 300000; n++) {
        const uint64_t s = lzh_zdslot_scratch_bytes(n);
        worst_seen = s > worst_seen ? s : worst_seen;
        if (n % 1000 == 0 || (n & (n - 1)) == 0 || (n > 0 && ((n - 1) & (n - 2)) == 0))
            CHECK(worst_seen <= lzh_zdslot_scratch_worst(n));
    }
    printf("zstd_dfast_slots_sweep: %zu chunks placed, all checks held\n", placed);
    return 0;
}
