// dense_check.cpp -- the host arithmetic of dense scoring (openwakeword_amd/csrc/owwhip_dense_host.h) as a plain host program: the header
// alone, no HIP, built with -fsanitize=address,undefined by tests/test_dense_cpu.py.  Window counts and row offsets for mixed T, tile
// counts at the edges of both tile sizes, the LDS geometry at every T 1..120 for passes of 1 and 2 nets (fits 160 KiB or routes to the
// fallback), the split of a group into passes, the staged
// rows' addresses and banks, slab arithmetic past 2^31 bytes, and every refusal.
// Output: "name value" lines the test reads; a failed self-check prints to stderr and exits 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "owwhip_dense_host.h"

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "dense_check: " __VA_ARGS__); fprintf(stderr, " [%s]\n", #cond); ++g_bad; } } while (0)

int main() {
    // ---- windows and offsets: heads of T = 5, 16, 22 on one handle
    {
        const int64_t t_max = 22, n_rows = 150;
        const int64_t nw = owd::n_win(n_rows, t_max);
        CHECK(nw == 129, "n_win %lld", (long long)nw);
        for (int64_t T : {5, 16, 22}) {
            const int64_t off = owd::row_offset(t_max, T);
            CHECK(off == t_max - T, "offset of T %lld", (long long)T);
            CHECK(off + (nw - 1) + T == n_rows, "T %lld: the last window ends at row %lld of %lld", (long long)T, (long long)(off + nw - 1 + T), (long long)n_rows);
            CHECK(off >= 0, "T %lld: window 0 starts at row %lld", (long long)T, (long long)off);
        }
        CHECK(owd::n_win(21, 22) == 0 && owd::n_win(22, 22) == 1, "one window needs t_max rows");
        printf("n_win_150_22 %lld\n", (long long)nw);
    }
    // ---- tiles at the edges, both tile sizes
    for (int64_t nw : {1, 127, 128, 129, 255, 256, 257, 261}) printf("tiles_%lld %lld %lld\n", (long long)nw, (long long)owd::tiles_per_seq(nw, 4), (long long)owd::tiles_per_seq(nw, 8));
    CHECK(owd::tiles_per_seq(1, 4) == 1 && owd::tiles_per_seq(127, 4) == 1 && owd::tiles_per_seq(128, 4) == 1 && owd::tiles_per_seq(129, 4) == 2, "tiles of 128");
    CHECK(owd::tiles_per_seq(256, 8) == 1 && owd::tiles_per_seq(257, 8) == 2 && owd::tiles_per_seq(129, 8) == 1, "tiles of 256");
    CHECK(owd::tile_rows(16, 4) == 143 && owd::tile_rows(1, 4) == 128 && owd::tile_rows(16, 8) == 271, "rows of a tile");

    // ---- LDS geometry: every T 1..120 (and on to 300) for passes of 1 and 2 nets either fits 160 KiB or routes to the fallback
    for (int nn = 1; nn <= owd::kMaxPassNets; ++nn) {
        const int64_t lim8 = owd::t_limit(nn, 8), lim4 = owd::t_limit(nn, 4);
        int fits_120 = 0, big_120 = 0;
        for (int64_t T = 1; T <= 300; ++T) {
            const owd::Geometry g = owd::geometry(nn, T);
            if (g.slots) {
                CHECK(g.waves == (T <= lim8 ? 8 : 4), "nn %d T %lld: %d waves", nn, (long long)T, g.waves);
                CHECK(g.slots >= owd::kMinSlots && g.slots <= owd::kMaxSlots, "nn %d T %lld: %d slots", nn, (long long)T, g.slots);
                CHECK(g.total <= owd::kLdsBytes, "nn %d T %lld: %lld bytes", nn, (long long)T, (long long)g.total);
                CHECK(g.staged == g.rows * owd::kRowWords * 4 && g.rows == 32 * g.waves + T - 1, "nn %d T %lld: staged rows", nn, (long long)T);
                CHECK(g.ring == (int64_t)g.slots * nn * 8192 && g.total == g.staged + g.ring, "nn %d T %lld: ring bytes", nn, (long long)T);
                // the ring is as deep as fits: one slot more would not
                CHECK(g.slots == owd::kMaxSlots || g.staged + (int64_t)(g.slots + 1) * nn * 8192 > owd::kLdsBytes, "nn %d T %lld: a deeper ring fits", nn, (long long)T);
                CHECK(T <= lim4, "nn %d: T %lld fits beyond the limit %lld", nn, (long long)T, (long long)lim4);
                // the last staged unit ends inside the allocation
                CHECK((int64_t)(owd::unit_word((int)g.rows - 1, 11) + owd::kUnitWords) * 4 <= g.staged, "nn %d T %lld: the last unit leaves the rows", nn, (long long)T);
                if (T <= 120) { ++fits_120; big_120 += g.waves == 8; }
            } else {
                CHECK(T > lim4, "nn %d: T %lld below the limit %lld takes the fallback", nn, (long long)T, (long long)lim4);
                CHECK(owd::staged_bytes(T, 4) + (int64_t)owd::kMinSlots * nn * 8192 > owd::kLdsBytes, "nn %d T %lld refused although two slots fit", nn, (long long)T);
            }
        }
        printf("t_limit_%d %lld %lld\nfits_to_120_%d %d %d\n", nn, (long long)lim8, (long long)lim4, nn, fits_120, big_120);
    }
    CHECK(!owd::geometry(0, 16).slots && !owd::geometry(3, 16).slots && !owd::geometry(1, 0).slots, "passes outside 1..2 nets or T < 1 take the fallback");
    printf("geo_1_16 %d %d\ngeo_2_16 %d %d\ngeo_2_73 %d %d\n", owd::geometry(1, 16).waves, owd::geometry(1, 16).slots, owd::geometry(2, 16).waves,
           owd::geometry(2, 16).slots, owd::geometry(2, 73).waves, owd::geometry(2, 73).slots);

    // ---- passes: at most two nets, a gated pair never split
    {
        struct Case { int n; int role[4]; int head[4]; int want[4][2]; int n_want; };
        const Case cases[] = {
            {1, {0}, {0}, {{0, 1}}, 1},
            {2, {0, 1}, {0, 0}, {{0, 2}}, 1},                                   // a gated pair
            {2, {0, 0}, {0, 1}, {{0, 2}}, 1},
            {3, {0, 1, 0}, {0, 0, 1}, {{0, 2}, {2, 1}}, 2},                     // pair, single (narrow3)
            {3, {0, 0, 1}, {0, 1, 1}, {{0, 1}, {1, 2}}, 2},                     // single, pair
            {4, {0, 0, 0, 1}, {0, 1, 2, 2}, {{0, 2}, {2, 2}}, 2},               // the three benchmark heads
            {4, {0, 0, 1, 0}, {0, 1, 1, 2}, {{0, 1}, {1, 2}, {3, 1}}, 3},       // single, pair, single
            {4, {0, 0, 0, 0}, {0, 1, 2, 3}, {{0, 2}, {2, 2}}, 2},
            {4, {0, 1, 0, 1}, {0, 0, 1, 1}, {{0, 2}, {2, 2}}, 2},
        };
        for (const Case& c : cases) {
            int got[4][2] = {};
            const int k = owd::split_passes(c.role, c.head, c.n, got);
            CHECK(k == c.n_want, "%d nets: %d passes", c.n, k);
            int next = 0;
            for (int i = 0; i < k; ++i) {
                CHECK(got[i][0] == c.want[i][0] && got[i][1] == c.want[i][1], "%d nets pass %d: (%d, %d)", c.n, i, got[i][0], got[i][1]);
                CHECK(got[i][0] == next && got[i][1] >= 1 && got[i][1] <= owd::kMaxPassNets, "%d nets pass %d leaves a gap", c.n, i);
                next += got[i][1];
            }
            CHECK(next == c.n, "%d nets: the passes cover %d", c.n, next);
        }
        printf("passes ok\n");
    }

    // ---- staged rows: the 16 positions of a tile, one row apart, read 16 distinct groups of four banks; units do not overlap
    for (int base = 0; base < 360; ++base)
        for (int unit = 0; unit < 12; ++unit) {
            std::set<int> banks;
            for (int pos = 0; pos < 16; ++pos) {
                const int w = owd::unit_word(base + pos, unit);
                CHECK(w % 4 == 0, "unit (%d, %d) is not 16-byte aligned", base + pos, unit);
                banks.insert((w % 64) / 4);
            }
            CHECK(banks.size() == 16, "rows %d..%d unit %d: %zu bank groups", base, base + 15, unit, banks.size());
        }
    {   // the lane groups the hardware serves a 16-byte read in (lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; lane =
        // 16 j + pos reads row base + pos, unit 4 c + j): no 4-bank slot is hit more than twice, two of sixteen are
        const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                   {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
        int worst = 0, doubled = 0;
        for (int base = 0; base < 64; ++base)
            for (int c = 0; c < 3; ++c)
                for (const auto& grp : groups) {
                    int hits[16] = {}, twice = 0;
                    for (int lane : grp) ++hits[(owd::unit_word(base + (lane & 15), owd::kstep_unit(c, lane >> 4)) % 64) / 4];
                    for (int h : hits) { worst = h > worst ? h : worst; twice += h == 2; }
                    doubled = twice > doubled ? twice : doubled;
                }
        CHECK(worst == 2 && doubled == 2, "lane groups: a slot is hit %d times, %d slots twice", worst, doubled);
        printf("lane_group_conflict %d %d\n", worst, doubled);
    }
    {
        std::set<int> seen;
        for (int row = 0; row < 3; ++row)
            for (int ks = 0; ks < 3; ++ks)
                for (int j = 0; j < 4; ++j) {
                    const int w = owd::unit_word(row, owd::kstep_unit(ks, j));
                    for (int k = 0; k < owd::kUnitWords; ++k) CHECK(seen.insert(w + k).second, "word %d written twice", w + k);
                    CHECK(w + owd::kUnitWords <= (row + 1) * owd::kRowWords, "unit (%d, %d, %d) leaves its row", row, ks, j);
                }
        CHECK(seen.size() == 3 * 96, "three rows hold %zu words", seen.size());
        CHECK(owd::kstep_unit(5, 3) == 11 && owd::kstep_unit(3, 0) == 0, "k-step units");
    }

    // ---- slabs: bounded, covering, 64-bit
    {
        const owd::Slab s = owd::slab(360000, 16);
        CHECK(s.bytes <= owd::kSlabBytes && s.windows == owd::kSlabBytes / (16 * 384) && s.n_slabs * s.windows >= 360000 && (s.n_slabs - 1) * s.windows < 360000, "slab of 360000 x 16");
        printf("slab_windows_16 %lld\nslab_count_360000_16 %lld\n", (long long)s.windows, (long long)s.n_slabs);
        const owd::Slab one = owd::slab(1, 120);
        CHECK(one.windows == 1 && one.n_slabs == 1 && one.bytes == 120 * 384, "a single window");
        const owd::Slab huge_T = owd::slab(10, 1 << 20);             // one window is larger than the budget: one window per slab
        CHECK(huge_T.windows == 1 && huge_T.n_slabs == 10 && huge_T.bytes == (int64_t)(1 << 20) * 384, "windows beyond the budget");
        // 40 million windows of T = 120: 1.8 TB of windows in all, past 2^31 bytes by far
        const int64_t total = 40000000ll;
        const owd::Slab big = owd::slab(total, 120);
        CHECK(big.bytes <= owd::kSlabBytes && big.n_slabs * big.windows >= total && total * 120 * 384 > (1ll << 40), "slabs of 1.8 TB");
        const owd::Slab wide_budget = owd::slab(total, 120, 1ll << 36);  // a 64 GiB budget: one slab is past 2^31 bytes and stays exact
        CHECK(wide_budget.bytes > (1ll << 31) && wide_budget.bytes == wide_budget.windows * 120 * 384 && wide_budget.windows <= INT32_MAX, "a slab past 2^31 bytes");
        printf("slab_big_bytes %lld\n", (long long)wide_budget.bytes);
        CHECK(owd::slab(0, 16).n_slabs == 0 && owd::slab(5, 0).n_slabs == 0, "empty requests");
        CHECK(owd::feats_bytes(8, 45015) == 8ull * 45015 * 384 && owd::out_bytes(1 << 20, 1 << 20, 32) == (1ull << 47), "64-bit sizes");
    }

    // ---- refusals
    {
        float x[4] = {};
        alignas(16) float al[8] = {};
        CHECK(owd::ready_check("f", false, false, 1) == OWW_ESTATE, "null handle");
        CHECK(owd::ready_check("f", true, false, 1) == OWW_ESTATE, "before commit");
        CHECK(owd::ready_check("f", true, true, 0) == OWW_EINVAL, "no fixed heads");
        CHECK(owd::ready_check("f", true, true, 3) == 0, "a committed handle with heads");
        CHECK(owd::shape_check("f", 21, 22) == OWW_EINVAL && owd::shape_check("f", 22, 22) == 0, "n_rows = t_max - 1");
        CHECK(owd::features_check("f", nullptr, 0, 1, 30, 16, 3, x, 0) == OWW_EINVAL, "null features");
        CHECK(owd::features_check("f", x, 0, 1, 30, 16, 3, nullptr, 0) == OWW_EINVAL, "null output");
        CHECK(owd::features_check("f", x, 0, 0, 30, 16, 3, x, 0) == OWW_EINVAL, "B = 0");
        CHECK(owd::features_check("f", x, 0, -1, 30, 16, 3, x, 0) == OWW_EINVAL, "B < 0");
        CHECK(owd::features_check("f", x, 0, 1, 15, 16, 3, x, 0) == OWW_EINVAL, "too few rows");
        CHECK(owd::features_check("f", al + 1, 1, 1, 30, 16, 3, x, 0) == OWW_EINVAL, "unaligned device features");
        CHECK(owd::features_check("f", al + 1, 0, 1, 30, 16, 3, x, 0) == 0, "host features need no alignment");
        CHECK(owd::features_check("f", al, 1, 3, 300, 22, 7, x, 1) == 0, "a good call");
        CHECK(owd::features_check("f", x, 0, INT32_MAX, INT32_MAX, 16, 32, x, 0) == OWW_ENOMEM, "2^62 rows");
        CHECK(owd::features_check("f", x, 0, 1 << 20, 1 << 20, 16, 32, x, 0) == OWW_ENOMEM, "2^47 bytes of scores");
        CHECK(owd::features_check("f", x, 0, 1 << 26, 4200, 16, 1, x, 0) == OWW_ENOMEM, "2^31 tiles and more");
        CHECK(owd::features_check("f", x, 0, 1 << 25, 8200, 16, 1, x, 0) == OWW_ENOMEM, "2^31 tiles of 128 within 1 TiB of features");
        CHECK(owd::clip_rows(511) == 0 && owd::clip_rows(12511) == 0 && owd::clip_rows(12512) == 1 && owd::clip_rows(64000) == 41, "embedding rows of a clip");
        CHECK(owd::clips_check("f", nullptr, 1, 64000, 8, 16, 3, x) == OWW_EINVAL, "null pcm");
        CHECK(owd::clips_check("f", x, 0, 64000, 8, 16, 3, x) == OWW_EINVAL, "no clips");
        CHECK(owd::clips_check("f", x, 9, 64000, 8, 16, 3, x) == OWW_EINVAL, "more clips than streams");
        CHECK(owd::clips_check("f", x, 2, 12000, 8, 16, 3, x) == OWW_EINVAL, "clips without an embedding");
        CHECK(owd::clips_check("f", x, 2, 12512 + 14 * 1280, 8, 16, 3, x) == OWW_EINVAL, "15 rows for t_max 16");
        CHECK(owd::clips_check("f", x, 2, 12512 + 15 * 1280, 8, 16, 3, x) == 0, "16 rows for t_max 16");
        CHECK(owd::clips_check("f", x, 8, 64000, 8, 16, 3, x) == 0, "a good call");
        printf("refusals ok\n");
    }
    if (g_bad) { fprintf(stderr, "dense_check: %d check(s) failed\n", g_bad); return 1; }
    printf("done 1\n");
    return 0;
}
