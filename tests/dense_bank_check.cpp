// dense_bank_check.cpp -- the host arithmetic of dense scoring over the head bank (openwakeword_amd/csrc/owwhip_dense_bank_host.h) as a
// plain host program: the header alone, no HIP, built with -fsanitize=address,undefined by tests/test_dense_bank_cpu.py.  The slice
// plan over 1 .. 4,097 heads x 1 .. 10^6 tiles (every (tile, head) covered exactly once, the grid inside one launch, the environment
// override), the staged row of every (t_s, T <= t_s, k-step) inside the geometry's rows, the statistics key's order, 64-bit sizes and
// every refusal.  Output: "name value" lines the test reads; a failed self-check prints to stderr and exits 1.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "owwhip_dense_bank_host.h"

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "dense_bank_check: " __VA_ARGS__); fprintf(stderr, " [%s]\n", #cond); ++g_bad; } } while (0)

// every (tile, head) of a plan is scored by exactly one block: walked block by block where the grid is small, by arithmetic otherwise
static void check_cover(const owd::BankPlan& p, int64_t n_heads, bool walk) {
    CHECK(p.hpw >= 1 && p.hpw <= n_heads, "hpw %d of %lld heads", p.hpw, (long long)n_heads);
    CHECK(p.slices == (n_heads + p.hpw - 1) / p.hpw && p.grid == p.tiles * p.slices, "slices %lld grid %lld", (long long)p.slices, (long long)p.grid);
    CHECK(p.grid >= 1 && p.grid <= owd::kMaxGrid, "grid %lld", (long long)p.grid);
    // the slices tile the list: first(s + 1) = first(s) + count(s), the last one ends at n_heads, none is empty
    const int s_last = (int)p.slices - 1;
    CHECK(owd::bank_slice_first(0, p.hpw) == 0, "slice 0 starts at %d", owd::bank_slice_first(0, p.hpw));
    CHECK(owd::bank_slice_first(s_last, p.hpw) + owd::bank_slice_count(s_last, p.hpw, (int)n_heads) == n_heads, "the last slice ends early or late");
    CHECK(owd::bank_slice_count(s_last, p.hpw, (int)n_heads) >= 1, "the last slice is empty");
    if (s_last > 0) CHECK(owd::bank_slice_count(s_last - 1, p.hpw, (int)n_heads) == p.hpw, "an inner slice is short");
    // the last block is the last slice's last tile
    CHECK(owd::bank_block_slice((int)(p.grid - 1), (int)p.tiles) == s_last && owd::bank_block_tile((int)(p.grid - 1), (int)p.tiles) == p.tiles - 1, "last block");
    if (!walk) return;
    std::vector<unsigned char> seen((size_t)(p.tiles * n_heads), 0);
    for (int64_t blk = 0; blk < p.grid; ++blk) {
        const int s = owd::bank_block_slice((int)blk, (int)p.tiles), t = owd::bank_block_tile((int)blk, (int)p.tiles);
        CHECK(s >= 0 && s < p.slices && t >= 0 && t < p.tiles, "block %lld -> slice %d tile %d", (long long)blk, s, t);
        const int i0 = owd::bank_slice_first(s, p.hpw), nh = owd::bank_slice_count(s, p.hpw, (int)n_heads);
        for (int r = 0; r < nh; ++r) {
            CHECK(i0 + r < n_heads, "block %lld reaches head %d", (long long)blk, i0 + r);
            if (i0 + r < n_heads) ++seen[(size_t)t * (size_t)n_heads + (size_t)(i0 + r)];
        }
    }
    int64_t wrong = 0;
    for (unsigned char c : seen) wrong += c != 1;
    CHECK(wrong == 0, "%lld (tile, head) pairs not covered exactly once (heads %lld tiles %lld hpw %d)", (long long)wrong, (long long)n_heads, (long long)p.tiles, p.hpw);
}

int main() {
    // ---- the slice plan
    {
        const int64_t heads[] = {1, 2, 3, 5, 7, 8, 9, 16, 17, 255, 256, 257, 1024, 4096, 4097};
        const int64_t seq_tiles[] = {1, 2, 3, 29, 30, 176, 1000, 99999, 1000000};
        int64_t plans = 0;
        for (int64_t n : heads)
            for (int64_t B : {1, 3, 8})
                for (int64_t st : seq_tiles)
                    for (int64_t forced : {0, 1, 2, 3, 5, 100000}) {
                        const int64_t nw = st * 256;            // t_s = 16: tiles of 256 windows
                        const owd::BankPlan p = owd::bank_plan(n, B, nw, 16, forced);
                        CHECK(p.hpw > 0 && p.seq_tiles == st && p.tiles == B * st && p.geo.waves == 8, "heads %lld B %lld tiles %lld: refused", (long long)n, (long long)B, (long long)st);
                        if (!p.hpw) continue;
                        check_cover(p, n, p.tiles * n <= 200000);
                        if (forced > 0 && n * p.tiles <= owd::kMaxGrid) CHECK(p.hpw == std::min<int64_t>(forced, n), "forced hpw %lld -> %d", (long long)forced, p.hpw);
                        if (!forced) CHECK(p.hpw <= std::max<int64_t>(owd::kBankHpwMax, (n * p.tiles + owd::kMaxGrid - 1) / owd::kMaxGrid + 1), "hpw %d", p.hpw);
                        ++plans;
                    }
        printf("plans %lld\n", (long long)plans);
        // the two measured shapes and the grid limit
        const owd::BankPlan big = owd::bank_plan(256, 8, 45000, 16), small = owd::bank_plan(256, 1, 7500, 16), one = owd::bank_plan(1, 1, 7500, 16);
        printf("plan_big %d %lld %lld\nplan_small %d %lld %lld\nplan_one %d %lld %lld\n", big.hpw, (long long)big.tiles, (long long)big.grid, small.hpw,
               (long long)small.tiles, (long long)small.grid, one.hpw, (long long)one.tiles, (long long)one.grid);
        CHECK(big.hpw == owd::kBankHpwMax && small.grid >= owd::kBankTargetGrid && one.hpw == 1 && one.grid == 30, "the measured shapes");
        const owd::BankPlan huge = owd::bank_plan(4097, 8, 256ll * 1000000, 16);      // 8 x 10^6 tiles x 4,097 heads: hpw grows past the cap
        CHECK(huge.hpw > owd::kBankHpwMax && huge.grid <= owd::kMaxGrid && huge.grid > owd::kMaxGrid / 2, "huge: hpw %d grid %lld", huge.hpw, (long long)huge.grid);
        check_cover(huge, 4097, false);
        printf("plan_huge %d %lld\n", huge.hpw, (long long)huge.grid);
        // refusals of the plan: no heads, no windows, rows that fit no tile, more tiles than one launch
        CHECK(!owd::bank_plan(0, 1, 100, 16).hpw && !owd::bank_plan(4, 1, 0, 16).hpw && !owd::bank_plan(4, 0, 100, 16).hpw, "empty plans");
        CHECK(!owd::bank_plan(4, 1, 100, owd::t_limit(1, 4) + 1).hpw && owd::bank_plan(4, 1, 100, owd::t_limit(1, 4)).hpw, "t_s beyond the LDS");
        CHECK(!owd::bank_plan(4, 3, (int64_t)INT32_MAX * 128, 120).hpw, "tiles beyond one launch");
        CHECK(owd::bank_plan(4, 1, 100, 113).geo.waves == 8 && owd::bank_plan(4, 1, 100, 114).geo.waves == 4 && owd::bank_plan(4, 1, 129, 114).seq_tiles == 2, "tile size edge");
        // the environment override
        unsetenv("OWW_DENSE_BANK_HPW");
        CHECK(owd::bank_hpw_env() == 0, "unset");
        for (const char* v : {"", "0", "-3", "x"}) { setenv("OWW_DENSE_BANK_HPW", v, 1); CHECK(owd::bank_hpw_env() == 0, "'%s' is no override", v); }
        setenv("OWW_DENSE_BANK_HPW", "5", 1);
        CHECK(owd::bank_hpw_env() == 5, "5");
        setenv("OWW_DENSE_BANK_HPW", "99999999999999", 1);
        CHECK(owd::bank_hpw_env() == INT32_MAX, "clamped");
        unsetenv("OWW_DENSE_BANK_HPW");
    }
    // ---- staged rows: every (t_s, T <= t_s, k-step, wave, tile, position) inside the geometry's rows; the first and the last one reached
    {
        int64_t n = 0;
        for (int t_s = 1; t_s <= (int)owd::t_limit(1, 4); ++t_s) {
            const owd::Geometry g = owd::geometry(1, t_s);
            CHECK(g.slots >= owd::kMinSlots, "t_s %d", t_s);
            int lo = INT32_MAX, hi = -1;
            for (int T = 1; T <= t_s; ++T)
                for (int ks = 0; ks < 3 * T; ++ks)
                    for (int wave : {0, g.waves - 1})
                        for (int t = 0; t < 2; ++t)
                            for (int pos : {0, 15}) {
                                const int row = owd::bank_staged_row(wave, t, pos, t_s, T, ks);
                                lo = std::min(lo, row); hi = std::max(hi, row);
                                // window (wave, t, pos) of a head of length T reads staged rows [window + t_s - T, window + t_s): row ks / 3 of them
                                if (row != 32 * wave + 16 * t + pos + (t_s - T) + ks / 3) ++g_bad;
                                if ((int64_t)(owd::unit_word(row, owd::kstep_unit(ks, 3)) + owd::kUnitWords) * 4 > g.staged) ++g_bad;
                                ++n;
                            }
            CHECK(lo == 0 && hi == g.rows - 1, "t_s %d: rows %d .. %d of %lld", t_s, lo, hi, (long long)g.rows);
        }
        CHECK(g_bad == 0, "a staged row leaves the geometry");
        printf("staged_rows %lld\n", (long long)n);
    }
    // ---- the statistics key orders like (score, -window)
    {
        const float sc[] = {0.0f, 1e-38f, 1e-9f, 0.25f, 0.5f, std::nextafter(0.5f, 1.0f), 0.99999994f, 1.0f};
        for (size_t a = 0; a < sizeof sc / sizeof *sc; ++a)
            for (size_t b = 0; b < sizeof sc / sizeof *sc; ++b)
                for (unsigned wa : {0u, 1u, 261u, 0x7ffffffeu})
                    for (unsigned wb : {0u, 1u, 261u, 0x7ffffffeu}) {
                        unsigned ba, bb;
                        memcpy(&ba, &sc[a], 4); memcpy(&bb, &sc[b], 4);
                        const unsigned long long ka = owd::stat_key(ba, wa), kb = owd::stat_key(bb, wb);
                        const bool want = sc[a] > sc[b] || (sc[a] == sc[b] && wa < wb);
                        CHECK((ka > kb) == want, "key order at %zu %zu %u %u", a, b, wa, wb);
                        CHECK(ka != 0 && owd::stat_key_bits(ka) == ba && owd::stat_key_window(ka) == wa, "key round trip");
                    }
        printf("keys ok\n");
    }
    // ---- sizes in 64-bit
    {
        CHECK(owd::out_bytes(8, 45000, 1024) == 8ull * 45000 * 1024 * 4 && owd::out_bytes(8, 45000, 1024) > (1ull << 30), "the matrix of the issue");
        CHECK(owd::stats_bytes(8, 1024) == 8ull * 1024 * 12, "statistics");
        CHECK(owd::stats_bytes(INT32_MAX, INT32_MAX) > (1ull << 63), "statistics past 2^63");
        printf("matrix_bytes %llu\n", (unsigned long long)owd::out_bytes(8, 45000, 1024));
    }
    // ---- every refusal
    {
        const char* fn = "check";
        alignas(16) static float buf[8];
        int32_t cnt[4]; float mx[4]; int32_t am[4];
        const int live[6] = {16, 0, 22, 5, 0, 120};
        int tm = -1;
        const int32_t ok_ids[] = {0, 2, 3, 2}, hole[] = {0, 1}, neg[] = {-1}, past[] = {6};
        CHECK(owd::bank_ready_check(fn, false, false, 1) == OWW_ESTATE && owd::bank_ready_check(fn, true, false, 1) == OWW_ESTATE, "not committed");
        CHECK(owd::bank_ready_check(fn, true, true, 0) == OWW_ESTATE && owd::bank_ready_check(fn, true, true, 1) == 0, "no bank");
        CHECK(owd::bank_ids_check(fn, ok_ids, 4, live, 6, &tm) == 0 && tm == 22, "duplicates pass, t_max = %d", tm);
        tm = -1;
        CHECK(owd::bank_ids_check(fn, ok_ids, 0, live, 6, &tm) == OWW_EINVAL && owd::bank_ids_check(fn, nullptr, 2, live, 6, &tm) == OWW_EINVAL, "n_ids < 1, null list");
        CHECK(owd::bank_ids_check(fn, ok_ids, -1, live, 6, &tm) == OWW_EINVAL, "n_ids < 0");
        CHECK(owd::bank_ids_check(fn, hole, 2, live, 6, &tm) == OWW_EINVAL && std::string(owp::g_err).find("1 is not a bank head") != std::string::npos, "a hole: %s", owp::g_err.c_str());
        CHECK(owd::bank_ids_check(fn, neg, 1, live, 6, &tm) == OWW_EINVAL && owd::bank_ids_check(fn, past, 1, live, 6, &tm) == OWW_EINVAL && tm == -1, "ids outside the bank");
        // the matrix entry
        CHECK(owd::bank_features_check(fn, buf, 0, 3, 40, 22, 4, buf, 0) == 0, "a valid call");
        CHECK(owd::bank_features_check(fn, buf, 0, 3, 21, 22, 4, buf, 0) == OWW_EINVAL && owd::bank_features_check(fn, buf, 0, 3, 22, 22, 4, buf, 0) == 0, "n_rows < t_max");
        CHECK(owd::bank_features_check(fn, nullptr, 0, 3, 40, 22, 4, buf, 0) == OWW_EINVAL && owd::bank_features_check(fn, buf, 0, 3, 40, 22, 4, nullptr, 0) == OWW_EINVAL, "null");
        CHECK(owd::bank_features_check(fn, buf, 0, 0, 40, 22, 4, buf, 0) == OWW_EINVAL, "B = 0");
        CHECK(owd::bank_features_check(fn, buf + 1, 1, 3, 40, 22, 4, buf, 0) == OWW_EINVAL && owd::bank_features_check(fn, buf + 1, 0, 3, 40, 22, 4, buf, 0) == 0, "misaligned device features");
        CHECK(owd::bank_features_check(fn, buf, 1, 3, 40, 22, 4, buf + 2, 1) == OWW_EINVAL && owd::bank_features_check(fn, buf, 1, 3, 40, 22, 4, buf + 4, 1) == 0, "misaligned device output");
        CHECK(owd::bank_features_check(fn, buf, 0, INT32_MAX, INT32_MAX, 22, 4, buf, 0) == OWW_ENOMEM && strstr(owp::g_err.c_str(), "bytes"), "features beyond 1 TiB");
        CHECK(owd::bank_features_check(fn, buf, 0, 8, 45021, 22, INT32_MAX, buf, 0) == OWW_ENOMEM && strstr(owp::g_err.c_str(), "bytes"), "a matrix beyond 1 TiB");
        CHECK(owd::bank_features_check(fn, buf, 0, 8, 45021, 22, 1024, buf, 0) == 0, "1.5 GB of scores fit");
        // the statistics entry
        const float thr_ok[4] = {0.0f, 0.5f, 1.0f, 2.0f}, thr_nan[4] = {0.5f, 0.5f, std::numeric_limits<float>::quiet_NaN(), 0.5f};
        CHECK(owd::bank_stats_check(fn, buf, 0, 3, 40, 22, 4, nullptr, cnt, mx, am) == 0 && owd::bank_stats_check(fn, buf, 0, 3, 40, 22, 4, thr_ok, cnt, mx, am) == 0, "valid");
        CHECK(owd::bank_stats_check(fn, buf, 0, 3, 40, 22, 4, thr_nan, cnt, mx, am) == OWW_EINVAL && strstr(owp::g_err.c_str(), "threshold 2"), "a NaN threshold");
        CHECK(owd::bank_stats_check(fn, buf, 0, 3, 21, 22, 4, nullptr, cnt, mx, am) == OWW_EINVAL, "n_rows < t_max");
        CHECK(owd::bank_stats_check(fn, nullptr, 0, 3, 40, 22, 4, nullptr, cnt, mx, am) == OWW_EINVAL && owd::bank_stats_check(fn, buf, 0, 3, 40, 22, 4, nullptr, nullptr, mx, am) == OWW_EINVAL &&
              owd::bank_stats_check(fn, buf, 0, 3, 40, 22, 4, nullptr, cnt, nullptr, am) == OWW_EINVAL && owd::bank_stats_check(fn, buf, 0, 3, 40, 22, 4, nullptr, cnt, mx, nullptr) == OWW_EINVAL, "null");
        CHECK(owd::bank_stats_check(fn, buf + 1, 1, 3, 40, 22, 4, nullptr, cnt, mx, am) == OWW_EINVAL, "misaligned device features");
        CHECK(owd::bank_stats_check(fn, buf, 0, 8, 45021, 22, 1 << 20, nullptr, cnt, mx, am) == 0, "a million heads' statistics fit where their matrix does not");
        CHECK(owd::bank_features_check(fn, buf, 0, 8, 45021, 22, 1 << 20, buf, 0) == OWW_ENOMEM, "... and the matrix is refused");
        CHECK(owd::bank_stats_check(fn, buf, 0, INT32_MAX, INT32_MAX, 22, 4, nullptr, cnt, mx, am) == OWW_ENOMEM, "features beyond 1 TiB");
        // (more tiles than one launch would need more than 2^38 rows: 1 TiB of features is reached first)
        CHECK(owd::bank_stats_check(fn, buf, 0, 17, INT32_MAX, 1, 1, nullptr, cnt, mx, am) == OWW_ENOMEM && strstr(owp::g_err.c_str(), "bytes"), "rows beyond one launch");
        printf("refusals %s\n", g_bad ? "bad" : "ok");
    }
    printf("done %d\n", g_bad ? 0 : 1);
    return g_bad ? 1 : 0;
}
