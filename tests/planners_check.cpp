// planners_check.cpp -- the host planners of the library as a plain host program: openwakeword_amd/csrc/owwhip_masked_host.h (the group
// lists of a masked step), owwhip_bank_host.h (the bank's routing table and refusals), owwhip_verifier_host.h (the per-stream verifier
// list and the assignment checks) and owwhip_state_host.h (record layout, group-block lists, refusals) -- the headers alone, no HIP,
// built with -fsanitize=address,undefined by tests/test_planners_cpu.py.  Every expectation is a definition restated here or a case
// worked by hand; every buffer a planner writes is malloc'ed at exactly the capacity it advertises.
//   planners_check                  masked, bank and state self-checks; "name value" lines the tests read (also for the Python mirrors)
//   planners_check verifier FILE    the verifier lists of the cases in FILE (tests/test_verifier_budget_cpu.py writes it), one line per entry
// A failed self-check prints to stderr and exits 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "owwhip_bank_host.h"
#include "owwhip_masked_host.h"
#include "owwhip_state_host.h"
#include "owwhip_verifier_host.h"

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "planners_check: " __VA_ARGS__); fprintf(stderr, " [%s]\n", #cond); ++g_bad; } } while (0)
static bool said(const char* what) { return owp::g_err == what; }

// ---------------------------------------------------------------------------------------------------------------- masked lists
// Definition: list k = the ascending distinct s / G_k over the streams with on[s] != 0, G = 1, 2, 4, 8, 16, packed back to back
static void masked_case(int S, const std::vector<uint8_t>& on, const char* what) {
    const size_t cap = owl::lists_capacity(S);
    int* out = (int*)malloc(cap * sizeof(int));
    uint8_t* mask = (uint8_t*)malloc(S);                 // (exactly S bytes: the 64-bit reads stay inside)
    for (size_t i = 0; i < cap; ++i) out[i] = -7;
    memcpy(mask, on.data(), S);
    int n[5]; size_t off[5];
    const int n_act = owl::build_lists(mask, S, out, n, off);
    std::vector<int> want;
    int want_act = 0;
    for (int k = 0; k < 5; ++k) {
        std::set<int> g;
        for (int s = 0; s < S; ++s) if (on[s]) g.insert(s >> k);
        CHECK(off[k] == want.size() && n[k] == (int)g.size(), "S %d %s: list %d at %zu with %d entries, want %zu and %zu", S, what, k, off[k], n[k], want.size(), g.size());
        want.insert(want.end(), g.begin(), g.end());
        if (k == 0) want_act = (int)g.size();
    }
    CHECK(n_act == want_act && want.size() <= cap, "S %d %s: %d participants, want %d", S, what, n_act, want_act);
    CHECK(want.empty() || memcmp(out, want.data(), want.size() * sizeof(int)) == 0, "S %d %s: the packed lists differ from the definition", S, what);
    if (want_act == 0) for (size_t i = 0; i < cap; ++i) CHECK(out[i] == -7, "S %d %s: word %zu written with nobody taking part", S, what, i);
    const int p = owl::participants(mask, S);
    CHECK(p == (want_act * 8 > S * 7 ? -1 : want_act), "S %d %s: participants() = %d with %d on", S, what, p, want_act);
    free(mask); free(out);
}
static void check_masked() {
    std::mt19937 rng(20250717);
    int cases = 0;
    for (int S : {1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 69}) {
        std::vector<uint8_t> m(S, 0);
        auto run = [&](const char* what) { masked_case(S, m, what); ++cases; };
        run("all off");
        m.assign(S, 1); run("all on");
        m.assign(S, 0); m[0] = 1; run("only stream 0");
        m.assign(S, 0); m[S - 1] = 1; run("only the last stream");
        m.assign(S, 0); for (int s = 0; s < S; s += 2) m[s] = 1; run("every second");
        m.assign(S, 0); for (int g = 0; g * 8 < S; ++g) m[std::min(S - 1, g * 8 + (3 * g) % 8)] = 1; run("one per group of 8");
        m.assign(S, 0); for (int s = S / 8 * 8; s < S; ++s) m[s] = 1; run("only the tail");
        m.assign(S, 0); for (int s = 0; s < S; ++s) m[s] = (uint8_t)(s % 3 == 0 ? 0x80 : s % 3 == 1 ? 0 : 0xff); run("bytes other than 1");
        for (double d : {0.125, 0.5, 0.875}) {
            for (int s = 0; s < S; ++s) m[s] = std::uniform_real_distribution<double>(0, 1)(rng) < d;
            run("random");
        }
    }
    // every size up to 300, 40 random masks each, densities from sparse to full
    for (int S = 1; S <= 300; ++S)
        for (int k = 0; k < 40; ++k) {
            std::vector<uint8_t> r(S);
            for (auto& b : r) b = (uint8_t)((int)(rng() % 40) <= k ? 1 + rng() % 255 : 0);
            masked_case(S, r, "sweep");
        }
    // the 7/8 rule
    std::vector<uint8_t> m(16, 1);
    m[3] = 0; CHECK(owl::participants(m.data(), 16) == -1, "15 of 16 use the dense launches");
    m[9] = 0; CHECK(owl::participants(m.data(), 16) == 14, "14 of 16 use the lists");
    m.assign(8, 1); CHECK(owl::participants(m.data(), 8) == -1, "8 of 8");
    m[5] = 0; CHECK(owl::participants(m.data(), 8) == 7, "7 of 8");
    m.assign(8, 0); CHECK(owl::participants(m.data(), 8) == 0, "nobody");
    printf("masked_cases %d\n", cases);
}

// ---------------------------------------------------------------------------------------------------------------- bank route
struct Head { bool live; int ht; size_t w1_bytes; };
static void route_invariants(const owb::Route& r, const std::vector<int>& sub, const std::vector<Head>& heads, const char* what) {
    std::multiset<int> got(r.entries.begin(), r.entries.end()), want;
    for (size_t i = 0; i < sub.size(); ++i) if (sub[i] >= 0) want.insert((int)i);
    CHECK(got == want, "%s: the entries are not the subscribed pairs, each once", what);
    CHECK(r.tile0[0] == 0 && r.tile0[1] == r.ntiles[0] && r.ntiles[0] + r.ntiles[1] == (int)r.tiles.size(), "%s: tile ranges", what);
    CHECK(r.entries_n[0] + r.entries_n[1] == (int)r.entries.size(), "%s: entry counts", what);
    double wb = 0.0;
    std::vector<int> covered(r.entries.size(), 0);
    for (int c = 0; c < 2; ++c)
        for (int t = r.tile0[c]; t < r.tile0[c] + r.ntiles[c]; ++t) {
            const owh::BankTile& bt = r.tiles[t];
            CHECK(bt.n >= 1 && bt.n <= 32 * r.wg[c] && bt.off >= 0 && bt.off + bt.n <= (int)r.entries.size() && bt.pad == 0, "%s: tile %d", what, t);
            CHECK(bt.head >= 0 && bt.head < (int)heads.size() && heads[bt.head].live && (heads[bt.head].ht == 8) == (c == 1), "%s: tile %d's head", what, t);
            if (bt.off < 0 || bt.off + bt.n > (int)r.entries.size()) continue;
            for (int i = bt.off; i < bt.off + bt.n; ++i) {
                CHECK(sub[r.entries[i]] == bt.head, "%s: tile %d reaches an entry of another head", what, t);
                CHECK(i == bt.off || r.entries[i] > r.entries[i - 1], "%s: tile %d's entries do not ascend", what, t);
                ++covered[i];
            }
            wb += (double)heads[bt.head].w1_bytes;
        }
    for (int c : covered) CHECK(c == 1, "%s: an entry lies in %d tiles", what, c);
    CHECK(wb == r.wbytes, "%s: %g weight bytes, the tiles' heads sum to %g", what, r.wbytes, wb);
}
// streams 0 .. sum(counts) - 1, K = 1: counts[b] consecutive streams subscribe to head b
static owb::Route route_counts(const std::vector<int>& counts, const std::vector<Head>& heads, std::vector<int>& sub, int forced = 0, bool sorted = true) {
    sub.clear();
    for (size_t b = 0; b < counts.size(); ++b) sub.insert(sub.end(), counts[b], (int)b);
    const owb::Route r = owb::route(sub.data(), (int)sub.size(), 1, heads.data(), (int)heads.size(), forced, sorted);
    route_invariants(r, sub, heads, "worked case");
    return r;
}
static std::string tile_sizes(const owb::Route& r) {
    std::string s;
    for (const auto& t : r.tiles) s += std::to_string(t.n) + (char)('A' + t.head) + " ";
    return s;
}
static void check_bank() {
    const size_t wA = 1000, wB = 7, wW = 50000;
    const std::vector<Head> one = {{true, 4, wA}}, two = {{true, 4, wA}, {true, 4, wB}}, mixed = {{true, 4, wA}, {true, 8, wW}};
    std::vector<int> sub;
    owb::Route r = route_counts({0}, one, sub);
    CHECK(r.ntiles[0] == 0 && r.ntiles[1] == 0 && r.wg[0] == 1 && r.wg[1] == 1 && r.wbytes == 0.0 && r.tiles.empty() && r.entries.empty(), "no subscriptions");
    r = route_counts({95}, one, sub);
    CHECK(r.wg[0] == 1 && tile_sizes(r) == "32A 32A 31A " && r.wbytes == 3.0 * wA && r.entries_n[0] == 95, "95 entries: %s", tile_sizes(r).c_str());
    r = route_counts({96}, one, sub);
    CHECK(r.wg[0] == 4 && tile_sizes(r) == "96A " && r.wbytes == 1.0 * wA, "96 entries: %s", tile_sizes(r).c_str());
    r = route_counts({128}, one, sub);
    CHECK(r.wg[0] == 4 && tile_sizes(r) == "128A ", "128 entries: %s", tile_sizes(r).c_str());
    r = route_counts({129}, one, sub);
    CHECK(r.wg[0] == 4 && tile_sizes(r) == "128A 1A " && r.wbytes == 2.0 * wA, "129 entries: %s", tile_sizes(r).c_str());
    r = route_counts({129, 1}, two, sub);
    CHECK(r.wg[0] == 1 && tile_sizes(r) == "32A 32A 32A 32A 1A 1B " && r.wbytes == 5.0 * wA + 1.0 * wB, "129 + 1 entries: %s", tile_sizes(r).c_str());
    CHECK(r.head_tiles[0].size() == 2 && r.head_tiles[0][0] == std::make_pair(0, 5) && r.head_tiles[0][1] == std::make_pair(5, 1), "per-head tile ranges");
    // largest first is a stable sort within the class; the per-head build keeps head order
    r = route_counts({1, 40}, two, sub);
    CHECK(tile_sizes(r) == "32B 8B 1A ", "sorted: %s", tile_sizes(r).c_str());
    r = route_counts({1, 40}, two, sub, 0, false);
    CHECK(tile_sizes(r) == "1A 32B 8B ", "head order: %s", tile_sizes(r).c_str());
    // a narrow and a wide head: each class its own wg, class 1 behind class 0
    r = route_counts({10, 200}, mixed, sub);
    CHECK(r.wg[0] == 1 && r.wg[1] == 4 && r.ntiles[0] == 1 && r.tile0[1] == 1 && r.ntiles[1] == 2 && tile_sizes(r) == "10A 128B 72B " && r.entries_n[1] == 200 &&
          r.wbytes == 1.0 * wA + 2.0 * wW, "narrow + wide: %s", tile_sizes(r).c_str());
    // forced waves per tile
    r = route_counts({96}, one, sub, 1);
    CHECK(r.wg[0] == 1 && r.wg[1] == 1 && tile_sizes(r) == "32A 32A 32A ", "forced 1: %s", tile_sizes(r).c_str());
    r = route_counts({95}, one, sub, 4);
    CHECK(r.wg[0] == 4 && r.wg[1] == 4 && tile_sizes(r) == "95A ", "forced 4: %s", tile_sizes(r).c_str());
    // a live head without subscribers is no group: 96 entries over one group, not two
    r = route_counts({96, 0}, two, sub);
    CHECK(r.wg[0] == 4 && tile_sizes(r) == "96A ", "an idle live head: %s", tile_sizes(r).c_str());
    // OWW_BANK_WG
    unsetenv("OWW_BANK_WG"); CHECK(owb::wg_env() == 0, "unset");
    setenv("OWW_BANK_WG", "4", 1); CHECK(owb::wg_env() == 4, "4");
    setenv("OWW_BANK_WG", "1", 1); CHECK(owb::wg_env() == 1, "1");
    setenv("OWW_BANK_WG", "2", 1); CHECK(owb::wg_env() == 0, "2 is not a choice");
    unsetenv("OWW_BANK_WG");
    // seeded random tables
    std::mt19937 rng(7);
    int tables = 0;
    for (int it = 0; it < 400; ++it) {
        const int S = 1 + (int)(rng() % 40), K = 1 + (int)(rng() % 3), cap = 1 + (int)(rng() % 6);
        std::vector<Head> heads(cap);
        for (auto& h : heads) h = Head{rng() % 4 != 0, rng() % 2 ? 8 : 4, (size_t)(1 + rng() % 100000)};
        std::vector<int> live;
        for (int b = 0; b < cap; ++b) if (heads[b].live) live.push_back(b);
        std::vector<int> tab((size_t)S * K, -1);
        if (!live.empty()) for (int& v : tab) if (rng() % 3) v = live[rng() % live.size()];
        const int forced = it % 5 == 0 ? (it % 10 ? 1 : 4) : 0;
        route_invariants(owb::route(tab.data(), S, K, heads.data(), cap, forced, it % 7 != 0), tab, heads, "random table");
        ++tables;
    }
    printf("bank_tables %d\n", tables);
    // the launch rule for the mirror (tests/head_windows.py::bank_waves): n entries spread over g heads of one class
    for (const auto& [n, g] : std::vector<std::pair<int, int>>{{95, 1}, {96, 1}, {191, 2}, {192, 2}}) {
        std::vector<int> counts(g, n / g);
        counts[0] += n - n / g * g;
        r = route_counts(counts, std::vector<Head>(g, Head{true, 4, wA}), sub);
        printf("bank_wg_%d_%d %d\n", n, g, r.wg[0]);
    }
    // refusals
    const int32_t good[8] = {0, 16, 64, 1, 1, 0, 0, 0};
    auto hdr = [&](int i, int v) { static int32_t h[8]; memcpy(h, good, sizeof h); h[i] = v; return (const int32_t*)h; };
    CHECK(owb::add_header_check(good, 16) == 0, "a good header");
    CHECK(owb::add_header_check(hdr(0, 1), 16) == OWW_EINVAL && said("oww_bank_add: gated heads are not accepted in the bank (load them as fixed heads)"), "kind 1");
    CHECK(owb::add_header_check(hdr(0, 2), 16) == OWW_EINVAL && said("oww_bank_add: multiclass heads are not accepted in the bank (load them as fixed heads)"), "kind 2");
    CHECK(owb::add_header_check(hdr(0, 3), 16) == OWW_EINVAL && said("oww_bank_add: recurrent heads are not accepted in the bank (load them as fixed heads)"), "kind 3");
    CHECK(owb::add_header_check(hdr(0, 9), 16) == OWW_EINVAL && said("oww_bank_add: unknown head kind 9"), "kind 9");
    CHECK(owb::add_header_check(hdr(3, 2), 16) == OWW_EINVAL && said("oww_bank_add: a bank head has one sigmoid output (n_out = 2)"), "n_out");
    CHECK(owb::add_header_check(hdr(5, 1), 16) == OWW_EINVAL && said("oww_bank_add: a bank head has exactly one hidden block (extra_blocks = 1)"), "extra_blocks");
    CHECK(owb::add_header_check(hdr(2, 129), 16) == OWW_EINVAL && said("oww_bank_add: hidden = 129 (a bank head has 1..128 hidden units)"), "hidden");
    CHECK(owb::add_header_check(hdr(2, 0), 16) == OWW_EINVAL && owb::add_header_check(hdr(2, 128), 16) == 0, "hidden 0, 128");
    CHECK(owb::add_header_check(hdr(1, 17), 16) == OWW_EINVAL && said("oww_bank_add: T = 17 exceeds the handle's feature ring (16 rows)"), "T");
    CHECK(owb::add_header_check(hdr(1, 0), 16) == OWW_EINVAL && owb::add_header_check(hdr(4, 0), 16) == 0, "T 0, no LayerNorm");
    CHECK(owb::add_header_check(hdr(4, 2), 16) == OWW_EINVAL && said("oww_bank_add: has_layernorm = 2"), "has_layernorm");
    const std::vector<Head> bank = {{true, 4, 1}, {false, 4, 0}, {true, 8, 1}};
    CHECK(owb::head_id_check("oww_bank_remove", 2, bank.data(), 3) == 0, "a head");
    CHECK(owb::head_id_check("oww_bank_remove", 1, bank.data(), 3) == OWW_EINVAL && said("oww_bank_remove: 1 is not a bank head"), "a hole");
    CHECK(owb::head_id_check("oww_bank_set_postproc", 3, bank.data(), 3) == OWW_EINVAL && said("oww_bank_set_postproc: 3 is not a bank head"), "past the bank");
    CHECK(owb::head_id_check("oww_bank_set_postproc", -1, bank.data(), 3) == OWW_EINVAL && said("oww_bank_set_postproc: -1 is not a bank head"), "negative");
    const int32_t st[2] = {4, 0}, st_bad[2] = {4, 5}, ids_ok[4] = {0, -1, 2, 2}, ids_hole[4] = {0, -1, 2, 1}, ids_neg[4] = {-2, 0, 0, 0};
    CHECK(owb::subscribe_check(st, 2, ids_ok, 5, 2, bank.data(), 3) == 0 && owb::subscribe_check(st, 0, nullptr, 5, 2, bank.data(), 3) == 0, "valid subscriptions");
    CHECK(owb::subscribe_check(st_bad, 2, ids_ok, 5, 2, bank.data(), 3) == OWW_EINVAL && said("oww_subscribe: stream id 5 out of range (0..4)"), "a stream past the handle");
    CHECK(owb::subscribe_check(st, 2, ids_hole, 5, 2, bank.data(), 3) == OWW_EINVAL && said("oww_subscribe: 1 is not a bank head (stream 0, slot 1)"), "a hole");
    CHECK(owb::subscribe_check(st, 2, ids_neg, 5, 2, bank.data(), 3) == OWW_EINVAL && said("oww_subscribe: -2 is not a bank head (stream 4, slot 0)"), "-2");
}

// ---------------------------------------------------------------------------------------------------------------- verifier list
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
// FILE: per case "case NAME S NL K n_pool n_ver", then fix [S NL], fix_thr (bit patterns, hex), bank [S K], bank_thr, pool_T [n_pool],
// ver_T [n_ver = NL, or 0: no handle-wide verifiers], ver_thr [n_ver]
static int verifier_lists(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "planners_check: cannot read %s\n", path); return 1; }
    char name[64];
    int S, NL, K, n_pool, n_ver;
    while (fscanf(f, " case %63s %d %d %d %d %d", name, &S, &NL, &K, &n_pool, &n_ver) == 6) {
        auto ints = [&](size_t n) { std::vector<int> v(n); for (int& x : v) if (fscanf(f, "%d", &x) != 1) ++g_bad; return v; };
        auto floats = [&](size_t n) { std::vector<float> v(n); for (float& x : v) { unsigned u = 0; if (fscanf(f, "%x", &u) != 1) ++g_bad; x = from_bits(u); } return v; };
        const std::vector<int> fix = ints((size_t)S * NL);
        const std::vector<float> fix_thr = floats((size_t)S * NL);
        const std::vector<int> bank = ints((size_t)S * K);
        const std::vector<float> bank_thr = floats((size_t)S * K);
        const std::vector<int> pool_T = ints(n_pool), ver_T = ints(n_ver);
        const std::vector<float> ver_thr = floats(n_ver);
        const std::vector<owk::SvEntry> list = owsv::sv_list(S, NL, K, fix, fix_thr, bank, bank_thr, pool_T, ver_T, ver_thr, owsv::count_assigned(fix, bank));
        CHECK(list.size() <= (size_t)S * (NL + K), "%s: %zu entries exceed the device list's capacity", name, list.size());
        printf("case %s %zu\n", name, list.size());
        for (const auto& e : list) printf("e %d %d %d %d %08x\n", e.s, e.col, e.T, e.v, bits(e.thr));
    }
    fclose(f);
    return g_bad ? 1 : 0;
}
static void check_assign() {
    const std::vector<int> pool_T = {16, 0, 5};                          // pool verifier 1 is free
    const int32_t st[2] = {0, 3}, v_ok[2] = {0, OWW_VERIFIER_NONE}, v_free[2] = {1, 0}, v_past[2] = {3, 0}, v_T[2] = {2, 0}, st_bad[2] = {0, 4};
    const float thr[2] = {0.25f, 0.5f};
    auto T16 = [](int) { return 16; };
    auto empty_slot = [](int s) { return s == 3 ? -1 : 16; };
    const char* fn = "oww_assign_verifiers";
    CHECK(owsv::assign_check(fn, false, 1, 2, st, 2, v_ok, thr, 4, pool_T, T16) == 0 && owsv::assign_check(fn, false, 1, 2, nullptr, 0, nullptr, nullptr, 4, pool_T, T16) == 0, "valid");
    CHECK(owsv::assign_check(fn, false, 2, 2, st, 2, v_ok, thr, 4, pool_T, T16) == OWW_EINVAL && said("oww_assign_verifiers: label 2 outside [0,2)"), "label");
    CHECK(owsv::assign_check("oww_bank_assign_verifiers", true, -1, 2, st, 2, v_ok, thr, 4, pool_T, T16) == OWW_EINVAL && said("oww_bank_assign_verifiers: slot -1 outside [0,2)"), "slot");
    CHECK(owsv::assign_check(fn, false, 0, 2, st, 2, v_ok, nullptr, 4, pool_T, T16) == OWW_EINVAL && said("oww_assign_verifiers: bad argument"), "null thresholds");
    CHECK(owsv::assign_check(fn, false, 0, 2, st, -1, v_ok, thr, 4, pool_T, T16) == OWW_EINVAL && said("oww_assign_verifiers: bad argument"), "n < 0");
    CHECK(owsv::assign_check(fn, false, 0, 2, st_bad, 2, v_ok, thr, 4, pool_T, T16) == OWW_EINVAL && said("oww_assign_verifiers: stream id 4 out of range (0..3)"), "stream");
    CHECK(owsv::assign_check(fn, false, 0, 2, st, 2, v_free, thr, 4, pool_T, T16) == OWW_EINVAL &&
          said("oww_assign_verifiers: 1 is not a pool verifier, OWW_VERIFIER_DEFAULT or OWW_VERIFIER_NONE (stream 0)"), "a free pool entry");
    CHECK(owsv::assign_check(fn, false, 0, 2, st, 2, v_past, thr, 4, pool_T, T16) == OWW_EINVAL, "past the pool");
    CHECK(owsv::assign_check(fn, false, 0, 2, st, 2, v_T, thr, 4, pool_T, T16) == OWW_EINVAL &&
          said("oww_assign_verifiers: verifier 2 has T = 5 feature rows, the model of stream 0's label 0 has T = 16"), "T mismatch");
    const int32_t v_two[2] = {0, 0};
    CHECK(owsv::assign_check("oww_bank_assign_verifiers", true, 1, 2, st, 2, v_two, thr, 4, pool_T, empty_slot) == OWW_EINVAL &&
          said("oww_bank_assign_verifiers: slot 1 of stream 3 is empty"), "an empty slot");
    // bookkeeping: the count follows the pairs that leave and return to the default
    std::vector<int> tab(4 * 2, OWW_VERIFIER_DEFAULT);
    std::vector<float> th(4 * 2, 0.f);
    long long n = 0;
    owsv::assign_apply(tab, th, n, 1, 2, st, 2, v_ok, thr);
    CHECK(n == 2 && tab[1] == 0 && tab[7] == OWW_VERIFIER_NONE && th[1] == 0.25f && th[7] == 0.5f && n == owsv::count_assigned(tab, {}), "two pairs assigned");
    const int32_t back[2] = {OWW_VERIFIER_DEFAULT, 2};
    owsv::assign_apply(tab, th, n, 1, 2, st, 2, back, thr);
    CHECK(n == 1 && tab[1] == OWW_VERIFIER_DEFAULT && tab[7] == 2 && n == owsv::count_assigned(tab, {}), "one back at the default, one reassigned");
}

// ---------------------------------------------------------------------------------------------------------------- state records
static std::vector<int> slice(const std::vector<int>& b, size_t at, size_t n) { return std::vector<int>(b.begin() + at, b.begin() + at + n); }
static void check_state_lists() {
    // worked case: levels {2, 8}, ids 9, 8, 3, 9
    const bool used[4] = {true, false, true, false};
    const int32_t ids[4] = {9, 8, 3, 9};
    std::vector<int> buf = {77};                                          // (a list already in the buffer: offsets are absolute)
    ows::StateList L;
    ows::state_list_build(used, ids, 4, buf, L);
    CHECK(L.n == 4 && L.ids_at == 1 && slice(buf, 1, 4) == std::vector<int>({9, 8, 3, 9}), "ids in record order");
    CHECK(L.n_groups[0] == 3 && L.items_at[0] == 5 && slice(buf, 5, 9) == std::vector<int>({1, -1, 2, 4, 1, 0, 4, -1, 3}), "level 2");
    CHECK(L.n_groups[1] == 0 && L.items_at[1] == 14, "level 4 is unused");
    CHECK(L.n_groups[2] == 3 && L.items_at[2] == 14 &&
          slice(buf, 14, 27) == std::vector<int>({0, -1, -1, -1, 2, -1, -1, -1, -1, 1, 1, 0, -1, -1, -1, -1, -1, -1, 1, -1, 3, -1, -1, -1, -1, -1, -1}), "level 8");
    CHECK(L.n_groups[3] == 0 && L.items_at[3] == 41 && buf.size() == 41, "level 16 is unused");
    // seeded lists: every record index once per used level, at place id % G of a block of group id / G
    std::mt19937 rng(11);
    int lists = 0;
    for (int it = 0; it < 300; ++it) {
        const int n = 1 + (int)(rng() % 40);
        std::vector<int32_t> v(n);
        if (it % 2) for (auto& x : v) x = (int32_t)(rng() % 69);
        else { std::vector<int32_t> all(69); for (int i = 0; i < 69; ++i) all[i] = i; std::shuffle(all.begin(), all.end(), rng); v.assign(all.begin(), all.begin() + n); }
        bool u[4];
        for (bool& b : u) b = rng() % 2;
        std::vector<int> b2;
        ows::StateList M;
        ows::state_list_build(u, v.data(), n, b2, M);
        for (int lv = 0; lv < 4; ++lv) {
            const int G = ows::kStateLevels[lv];
            CHECK(u[lv] || M.n_groups[lv] == 0, "an unused level has blocks");
            std::vector<int> seen(n, 0);
            for (int k = 0; k < M.n_groups[lv]; ++k) {
                const size_t at = M.items_at[lv] + (size_t)k * (G + 1);
                CHECK(at + G < b2.size(), "a block past the buffer");
                if (at + G >= b2.size()) break;
                for (int p = 0; p < G; ++p) {
                    const int i = b2[at + 1 + p];
                    if (i < 0) continue;
                    CHECK(i < n && v[i] / G == b2[at] && v[i] % G == p, "record %d sits at place %d of group %d", i, p, b2[at]);
                    if (i < n) ++seen[i];
                }
            }
            if (u[lv]) for (int c : seen) CHECK(c == 1, "a record index appears %d times at level %d", c, G);
            if (u[lv] && it % 2 == 0) {                                      // no repeats: one block per touched group
                std::set<int> groups;
                for (int x : v) groups.insert(x / G);
                CHECK(M.n_groups[lv] == (int)groups.size(), "%d blocks for %zu touched groups", M.n_groups[lv], groups.size());
            }
        }
        ++lists;
    }
    printf("state_lists %d\n", lists);
}
static void check_state_refusals() {
    const int32_t neg[2] = {0, -1}, past[2] = {69, 0}, twice[3] = {5, 7, 5}, ok[3] = {68, 0, 5};
    CHECK(ows::state_check_ids(69, "oww_state_import", "the", ok, 3, true) == 0, "valid ids");
    CHECK(ows::state_check_ids(69, "oww_state_export", "the", neg, 2, false) == OWW_EINVAL && said("oww_state_export: the stream id -1 out of range (0..68)"), "-1");
    CHECK(ows::state_check_ids(69, "oww_move_streams", "source", past, 2, false) == OWW_EINVAL && said("oww_move_streams: source stream id 69 out of range (0..68)"), "S");
    CHECK(ows::state_check_ids(69, "oww_move_streams", "destination", twice, 3, true) == OWW_EINVAL && said("oww_move_streams: destination stream id 5 is listed twice"), "a repeat");
    CHECK(ows::state_check_ids(69, "oww_move_streams", "source", twice, 3, false) == 0, "a repeat where repeats are allowed");
    const uint64_t fp = 0x0123456789abcdefull;
    const uint32_t good[8] = {ows::kMagic, ows::kLayoutVersion, 49344, 0, (uint32_t)fp, (uint32_t)(fp >> 32), 0, 0};
    uint32_t h[16];
    auto two = [&](int i, uint32_t v) { memcpy(h, good, 32); memcpy(h + 8, good, 32); h[8 + i] = v; return (const uint32_t*)h; };
    CHECK(ows::state_check_headers(12336, fp, two(3, 0), 2) == 0, "two good headers");
    CHECK(ows::state_check_headers(12336, fp, two(0, 0xdeadbeefu), 2) == OWW_EINVAL &&
          said("oww_state_import: record 1 does not start with a stream state header (magic deadbeef)"), "magic");
    CHECK(ows::state_check_headers(12336, fp, two(1, 2), 2) == OWW_EINVAL && said("oww_state_import: record 1 has record layout version 2, this library reads version 1"), "version");
    const char* other = "oww_state_import: record 1 comes from another configuration: the record carries fingerprint %016llx and %u bytes, this handle has "
                        "fingerprint 0123456789abcdef and 49344 bytes (kernel family, ring sizes, bank slots, VAD, calibration scales or weights differ)";
    char want[512];
    snprintf(want, sizeof want, other, (unsigned long long)fp, 49340u);
    CHECK(ows::state_check_headers(12336, fp, two(2, 49340), 2) == OWW_EINVAL && said(want), "size: %s", owp::g_err.c_str());
    snprintf(want, sizeof want, other, (unsigned long long)(fp ^ 1), 49344u);
    CHECK(ows::state_check_headers(12336, fp, two(4, (uint32_t)fp ^ 1u), 2) == OWW_EINVAL && said(want), "fingerprint: %s", owp::g_err.c_str());
    CHECK(ows::kMagic == 0x5354574fu && ows::kLayoutVersion == 1u && ows::kHeaderWords == 8, "the record constants");
}
// the default register-resident configuration (3 fixed heads, feature ring 16; with_vad: the VAD network too), sections in the handle's order
static void check_state_layout() {
    static uint32_t live_word;
    static float live_f;
    const char* names[owp::N_STATE] = {"hist_mel", "hist2", "B:b", "B:d", "C:b", "C:d", "D:b", "D:d", "E:b", "E:d", "hist19"};
    for (int with_vad = 0; with_vad < 2; ++with_vad) {
        std::vector<ows::FlatSection> flat;
        std::vector<ows::GroupSection> group;
        std::vector<std::string> fname, gname;
        auto add = [&](const char* nm, uint32_t stride, uint32_t len, bool have = true) { flat.push_back(ows::FlatSection{have ? &live_word : nullptr, stride, len, 0, 0}); if (have && len) fname.push_back(nm); };
        const uint32_t NL = 3, K = 0;
        for (int a = 0; a < owp::N_STATE; ++a) if (owp::kStateSpgRr[a] == 1) add(names[a], owp::kStateLenRr[a], owp::kStateLenRr[a]);
        add("pcm_tail", 240, 240); add("feature_ring", 16 * 96, 16 * 96); add("score_ring", NL * OWW_SCORE_RING, NL * OWW_SCORE_RING);
        add("raw", NL, NL); add("scores", NL, NL); add("frame_counter", 1, 1); add("prediction_counter", 1, 1); add("vad_ring", 8, 8); add("vad_counter", 1, 1);
        if (with_vad) add("vad_last", 1, 1);
        add("no_buffer", 4, 4, false); add("bank_raw", K, K);                    // dropped: no buffer, no words
        for (int a = 0; a < owp::N_STATE; ++a)
            if (owp::kStateSpgRr[a] > 1) {
                group.push_back(ows::GroupSection{&live_f, owp::kStateSpgRr[a], 16 / owp::kStateSpgRr[a], true, (uint32_t)(owp::kStateLenRr[a] * owp::kStateSpgRr[a]), 0});
                gname.push_back(names[a]);
            }
        if (with_vad) { group.push_back(ows::GroupSection{&live_f, 16, 1, true, 4096, 0}); gname.push_back("vad_hc"); }
        ows::Layout L;
        CHECK(ows::layout(flat, group, L) == 0 && flat.size() == fname.size(), "the default layout is refused, or a dropped section stayed");
        // by hand: 8 header words + 5,184 of histories + 240 + 1,536 + 92 + 4 x 4 + 8 + 4 = 7,088 flat; + 5,248 grouped = 12,336 words
        CHECK(L.flat_quads == (7088u + (with_vad ? 4u : 0u)) / 4 && L.record_words == 12336u + (with_vad ? 4u + 256u : 0u), "record of %u words", L.record_words);
        uint32_t at = ows::kHeaderWords;
        for (size_t i = 0; i < flat.size(); ++i) {
            CHECK(flat[i].off == at && flat[i].off % 4 == 0 && flat[i].vec == (flat[i].len % 4 == 0), "flat section %s at %u", fname[i].c_str(), flat[i].off);
            at += (flat[i].len + 3) / 4 * 4;
            printf("off%d %s %u %u\n", with_vad, fname[i].c_str(), flat[i].off, flat[i].len);
        }
        for (size_t i = 0; i < group.size(); ++i) {
            const uint32_t words = group[i].block_words / (uint32_t)group[i].spg;
            CHECK(group[i].off == at, "group section %s at %u", gname[i].c_str(), group[i].off);
            at += words;
            printf("off%d %s %u %u\n", with_vad, gname[i].c_str(), group[i].off, words);
        }
        printf("record_bytes%d %u\n", with_vad, L.record_words * 4);
    }
    // the fp32 family's position counts are layouts too; a block that is no multiple of 16 R words, an unknown ppr, too many positions are not
    const char* msg = "state records: a group block of %u words, %d streams and %d positions per stream is not a layout the record kernels know";
    char want[256];
    auto one = [&](int spg, int ppr, uint32_t bw) {
        std::vector<ows::FlatSection> f; std::vector<ows::GroupSection> g = {ows::GroupSection{&live_f, spg, ppr, false, bw, 0}};
        ows::Layout L; snprintf(want, sizeof want, msg, bw, spg, ppr);
        return ows::layout(f, g, L);
    };
    CHECK(one(8, 1, 64) == 0 && one(8, 2, 32) == 0 && one(2, 8, 16) == 0, "known layouts");
    CHECK(one(8, 1, 96) == OWW_ESTATE && said(want), "96 words at R = 4");
    CHECK(one(8, 2, 48) == OWW_ESTATE && said(want), "48 words at R = 2");
    CHECK(one(2, 8, 24) == OWW_ESTATE && said(want), "24 words at R = 1");
    CHECK(one(4, 3, 64) == OWW_ESTATE && said(want) && one(4, 8, 64) == OWW_ESTATE && said(want) && one(4, 0, 64) == OWW_ESTATE, "unknown position counts");
    // fingerprint: FNV-1a over the words and blobs in the documented order, restated
    const int sl[2] = {64, 2048}, e[20] = {1, 2, 3};
    const float mel[3] = {1.f, 2.f, 3.f}, w[2] = {4.f, 5.f};
    const std::vector<ows::HeadPrint> heads = {{{0, 16, 32, 1, 1, 1}, {w, sizeof w}}};
    auto fnv = [](uint64_t h, const void* p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; } return h; };
    // version, family, interleave | state lengths | TR, NL, K, vad | 20 layer exponents | the feature exponent
    std::vector<int32_t> words = {(int32_t)ows::kLayoutVersion, 3, 1, 64, 2048, 16, 3, 2, 1, 1, 2, 3};
    words.resize(words.size() + 17, 0);
    words.push_back(-7);
    uint64_t fw = fnv(1469598103934665603ull, words.data(), words.size() * 4);
    fw = fnv(fw, mel, sizeof mel); fw = fnv(fw, heads[0].hdr, 24); fw = fnv(fw, w, sizeof w);
    const uint64_t got = ows::fingerprint(3, true, sl, 2, 16, 3, 2, true, e, -7, {mel, sizeof mel}, {nullptr, 0}, heads, {nullptr, 0});
    CHECK(got == fw, "fingerprint %016llx, restated %016llx", (unsigned long long)got, (unsigned long long)fw);
    CHECK(ows::fingerprint(1, true, sl, 2, 16, 3, 2, true, nullptr, -7, {mel, sizeof mel}, {nullptr, 0}, heads, {nullptr, 0}) != got, "the family and scales count");
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "verifier")) return verifier_lists(argv[2]);
    check_masked();
    check_bank();
    check_assign();
    check_state_lists();
    check_state_refusals();
    check_state_layout();
    printf("done %d\n", g_bad ? 0 : 1);
    return g_bad ? 1 : 0;
}
