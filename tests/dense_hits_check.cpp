// dense_hits_check.cpp -- the host side of the ordered hit lists (openwakeword_amd/csrc/owwhip_dense_hits_host.h) as a plain host program:
// the header alone, no HIP, built with -fsanitize=address,undefined by tests/test_dense_hits_cpu.py.  Mask geometry and 64-bit sizes at
// the word edges and at 2^31-scale products, the win_offset table for mixed T, every refusal and its message, the scalar compaction
// (which dense_hits_compact_kernel implements) on masks with empty and full words, a set last bit of a sequence and caps of 1, the total
// and the total - 1, and the slab plan's cover and bounds.
// Output: "name value" lines the test reads; a failed self-check prints to stderr and exits 1.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "owwhip_dense_hits_host.h"

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "dense_hits_check: " __VA_ARGS__); fprintf(stderr, " [%s]\n", #cond); ++g_bad; } } while (0)
static bool says(const char* part) { return owp::g_err.find(part) != std::string::npos; }

// the definition, once more and naively: every (seq, window) whose bit is set, in order
static std::vector<owdh::Pos> naive(const std::vector<uint32_t>& words, int64_t B, int64_t wps) {
    std::vector<owdh::Pos> v;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t w = 0; w < wps * 32; ++w)
            if ((words[(size_t)(b * wps + w / 32)] >> (w % 32)) & 1u) v.push_back(owdh::Pos{(int32_t)b, (int32_t)w});
    return v;
}
static void check_compaction(const char* name, const std::vector<uint32_t>& words, int64_t B, int64_t wps) {
    const std::vector<owdh::Pos> all = naive(words, B, wps);
    const int64_t total = (int64_t)all.size();
    for (int64_t cap : {(int64_t)1, total, total - 1, total + 3, (int64_t)7}) {
        if (cap < 1) continue;
        std::vector<owdh::Pos> out((size_t)cap + 2, owdh::Pos{-77, -77});            // two guard slots behind the cap
        const int64_t got = owdh::compact(words.data(), B, wps, cap, out.data());
        CHECK(got == total, "%s cap %lld: total %lld, expected %lld", name, (long long)cap, (long long)got, (long long)total);
        const int64_t stored = std::min(cap, total);
        for (int64_t r = 0; r < stored; ++r)
            CHECK(out[(size_t)r].seq == all[(size_t)r].seq && out[(size_t)r].window == all[(size_t)r].window, "%s cap %lld: slot %lld = (%d, %d)", name,
                  (long long)cap, (long long)r, out[(size_t)r].seq, out[(size_t)r].window);
        for (int64_t r = stored; r < cap + 2; ++r) CHECK(out[(size_t)r].seq == -77, "%s cap %lld: slot %lld behind the list was written", name, (long long)cap, (long long)r);
    }
    printf("compact_%s %lld\n", name, (long long)total);
}

int main() {
    // ---- mask geometry at the word edges
    for (int64_t nw : {1, 31, 32, 33, 257}) {
        const int64_t wps = owdh::words_per_seq(nw);
        CHECK(wps * 32 >= nw && (wps - 1) * 32 < nw, "n_win %lld: %lld words", (long long)nw, (long long)wps);
        for (int64_t B : {1, 3, 5}) {
            const int64_t cs = owdh::col_stride(B, nw);
            CHECK(cs % 4 == 0 && cs >= B * wps && cs < B * wps + 4, "n_win %lld B %lld: column stride %lld", (long long)nw, (long long)B, (long long)cs);
            CHECK(owdh::mask_bytes(7, B, nw) == 7ull * (uint64_t)cs * 4u, "n_win %lld B %lld: mask bytes", (long long)nw, (long long)B);
        }
        printf("wps_%lld %lld\n", (long long)nw, (long long)wps);
    }
    // 1,024 heads at the usual 2^18-row chunk: 32 MB
    CHECK(owdh::mask_bytes(1024, 1, (1 << 18) - 15) == 1024ull * 8192 * 4, "the mask of 1,024 heads over 2^18 rows");
    printf("mask_bytes_1024 %llu\n", (unsigned long long)owdh::mask_bytes(1024, 1, (1 << 18) - 15));
    // ---- 64-bit sizes at 2^31-scale products
    CHECK(owdh::mask_bytes(1 << 20, 1 << 10, 1 << 20) == (1ull << 20) * (1ull << 25) * 4u, "2^47 bytes of mask");
    CHECK(owdh::hits_bytes(1 << 15, 1 << 20) == (1ull << 39), "2^39 bytes of records");
    CHECK(owdh::cap_eff(1 << 20, 3, 261) == 783 && owdh::cap_eff(5, 3, 261) == 5, "the device's slots per column");
    {
        const int T3[3] = {120, 120, 120};
        CHECK(owdh::windows_bytes(T3, 3, 1 << 20) == 3ull * 120 * 384 * (1ull << 20), "windows past 2^31 bytes");
        int64_t off[4];
        owdh::win_offsets(T3, 3, 1 << 20, off);
        CHECK(off[3] == 3ll * 120 * 96 * (1ll << 20) && off[3] > (1ll << 31), "win_offset past 2^31 floats");
        printf("win_total_big %lld\n", (long long)off[3]);
    }
    // ---- win_offset for mixed T
    {
        const int T[4] = {5, 16, 22, 1};
        int64_t off[5];
        owdh::win_offsets(T, 4, 10, off);
        CHECK(off[0] == 0 && off[1] == 10 * 5 * 96 && off[2] == off[1] + 10 * 16 * 96 && off[3] == off[2] + 10 * 22 * 96 && off[4] == off[3] + 10 * 96, "mixed T");
        CHECK((uint64_t)off[4] * 4 == owdh::windows_bytes(T, 4, 10), "the table's end is the buffer's size");
        printf("win_offset_mixed %lld %lld %lld %lld %lld\n", (long long)off[0], (long long)off[1], (long long)off[2], (long long)off[3], (long long)off[4]);
    }
    // ---- refusals and their messages
    {
        float x[4] = {};
        alignas(16) float al[8] = {};
        int32_t ns[4]; int64_t nt[4];
        CHECK(owdh::cap_check("f", 0) == OWW_EINVAL && says("cap = 0") && says("1048576"), "cap 0: %s", owp::g_err.c_str());
        CHECK(owdh::cap_check("f", (1 << 20) + 1) == OWW_EINVAL && says("cap = 1048577"), "cap above 1 << 20");
        CHECK(owdh::cap_check("f", 1) == 0 && owdh::cap_check("f", 1 << 20) == 0, "the cap's ends");
        CHECK(owdh::layout_check("f", 4, nullptr) == OWW_EINVAL && says("win_offset"), "null win_offset");
        CHECK(owdh::layout_check("f", 0, nt) == OWW_EINVAL && owdh::layout_check("f", 4, nt) == 0, "layout");
        CHECK(owdh::features_check("fn_name", x, 0, 1, 30, 16, 3, 4, nullptr, ns, nt, nullptr, 0) == OWW_EINVAL && says("fn_name") && says("required"), "null hits");
        CHECK(owdh::features_check("f", x, 0, 1, 30, 16, 3, 4, x, nullptr, nt, nullptr, 0) == OWW_EINVAL, "null n_stored");
        CHECK(owdh::features_check("f", x, 0, 1, 30, 16, 3, 4, x, ns, nullptr, nullptr, 0) == OWW_EINVAL, "null n_total");
        CHECK(owdh::features_check("f", nullptr, 0, 1, 30, 16, 3, 4, x, ns, nt, nullptr, 0) == OWW_EINVAL && says("null features"), "null features");
        CHECK(owdh::features_check("f", x, 0, 0, 30, 16, 3, 4, x, ns, nt, nullptr, 0) == OWW_EINVAL, "B = 0");
        CHECK(owdh::features_check("f", x, 0, 1, 15, 16, 3, 4, x, ns, nt, nullptr, 0) == OWW_EINVAL && says("less than one window"), "n_rows < t_max");
        CHECK(owdh::features_check("f", x, 0, 1, 30, 16, 3, 0, x, ns, nt, nullptr, 0) == OWW_EINVAL, "cap 0 through the entry's check");
        CHECK(owdh::features_check("f", al + 1, 1, 1, 30, 16, 3, 4, x, ns, nt, nullptr, 0) == OWW_EINVAL, "misaligned device features");
        CHECK(owdh::features_check("f", x, 0, 1, 30, 16, 3, 4, x, ns, nt, al + 1, 1) == OWW_EINVAL && says("16-byte aligned"), "misaligned device windows");
        CHECK(owdh::features_check("f", x, 0, 1, 30, 16, 3, 4, x, ns, nt, al + 1, 0) == 0, "host windows need no alignment");
        CHECK(owdh::features_check("f", x, 0, 3, 300, 22, 7, 4096, x, ns, nt, al, 1) == 0, "a good call");
        CHECK(owdh::features_check("f", x, 0, INT32_MAX, INT32_MAX, 16, 32, 4, x, ns, nt, nullptr, 0) == OWW_ENOMEM && says("bytes of features"), "2^62 rows");
        CHECK(owdh::features_check("f", x, 0, 1 << 10, 1 << 20, 16, 1 << 20, 4, x, ns, nt, nullptr, 0) == OWW_ENOMEM && says("bytes of hit mask"), "2^47 bytes of mask: %s",
              owp::g_err.c_str());
        CHECK(owdh::features_check("f", x, 0, 1 << 25, 8200, 16, 1, 4, x, ns, nt, nullptr, 0) == OWW_ENOMEM, "2^31 tiles");
        CHECK(owdh::clips_check("f", nullptr, 1, 64000, 8, 16, 3, 4, x, ns, nt, nullptr, 0) == OWW_EINVAL, "null pcm");
        CHECK(owdh::clips_check("f", x, 9, 64000, 8, 16, 3, 4, x, ns, nt, nullptr, 0) == OWW_EINVAL, "more clips than streams");
        CHECK(owdh::clips_check("f", x, 2, 12000, 8, 16, 3, 4, x, ns, nt, nullptr, 0) == OWW_EINVAL && says("no embedding"), "clips without an embedding");
        CHECK(owdh::clips_check("f", x, 2, 12512 + 14 * 1280, 8, 16, 3, 4, x, ns, nt, nullptr, 0) == OWW_EINVAL, "15 rows for t_max 16");
        CHECK(owdh::clips_check("f", x, 2, 64000, 8, 16, 3, (1 << 20) + 1, x, ns, nt, nullptr, 0) == OWW_EINVAL, "cap above the limit");
        CHECK(owdh::clips_check("f", x, 8, 64000, 8, 16, 3, 4, x, ns, nt, nullptr, 0) == 0, "a good clip call");
        const float thr[3] = {0.5f, NAN, 0.1f};
        CHECK(owdh::bank_thresholds_check("f", thr, 3) == OWW_EINVAL && says("threshold 1 is NaN"), "a NaN bank threshold");
        CHECK(owdh::bank_thresholds_check("f", thr, 1) == 0 && owdh::bank_thresholds_check("f", nullptr, 3) == 0, "good thresholds");
        printf("refusals ok\n");
    }
    // ---- the scalar compaction
    {
        // B = 3, n_win = 70 (three words, the last holds 6 windows): empty words, a full word, the last bit of a sequence
        const int64_t B = 3, wps = 3;
        std::vector<uint32_t> m((size_t)(B * wps), 0u);
        m[1] = 0xffffffffu;                     // sequence 0, windows 32 .. 63
        m[2] = 1u << 5;                         // sequence 0, window 69: the last window of the sequence
        m[6] = 1u | (1u << 31);                 // sequence 2, windows 0 and 31
        m[8] = (1u << 5) | 1u;                  // sequence 2, windows 64 and 69
        check_compaction("edges", m, B, wps);
        std::vector<uint32_t> none((size_t)(B * wps), 0u);
        check_compaction("none", none, B, wps);
        std::vector<uint32_t> full((size_t)(B * wps), 0xffffffffu);
        check_compaction("full", full, B, wps);
        std::vector<uint32_t> one(1, 1u);       // n_win = 1
        check_compaction("single", one, 1, 1);
        std::vector<uint32_t> rnd(5 * 9);
        uint32_t s = 12345u;
        for (uint32_t& w : rnd) { s = s * 1664525u + 1013904223u; w = s & (s >> 3) & (s << 5); }
        check_compaction("random", rnd, 5, 9);
    }
    // ---- the slab plan: covers [0, n) in order, every piece within the budget
    {
        for (int64_t n : {(int64_t)1, (int64_t)100, (int64_t)43690, (int64_t)43691, (int64_t)(1 << 20)})
            for (int64_t T : {1, 16, 120}) {
                const std::vector<owdh::HitSlab> plan = owdh::slab_plan(n, T);
                int64_t next = 0;
                for (const owdh::HitSlab& p : plan) {
                    CHECK(p.first == next && p.n >= 1, "n %lld T %lld: a piece starts at %lld, expected %lld", (long long)n, (long long)T, (long long)p.first, (long long)next);
                    CHECK(p.n * T * 384 <= owd::kSlabBytes, "n %lld T %lld: a piece of %lld windows", (long long)n, (long long)T, (long long)p.n);
                    next += p.n;
                }
                CHECK(next == n, "n %lld T %lld: the plan covers %lld", (long long)n, (long long)T, (long long)next);
            }
        CHECK(owdh::slab_plan(0, 16).empty(), "no hits, no slab");
        const std::vector<owdh::HitSlab> small = owdh::slab_plan(10, 16, 3 * 16 * 384);
        CHECK(small.size() == 4 && small[3].first == 9 && small[3].n == 1, "a budget of three windows");
        printf("slab_pieces_2e20_120 %zu\n", owdh::slab_plan(1 << 20, 120).size());
    }
    if (g_bad) { fprintf(stderr, "dense_hits_check: %d check(s) failed\n", g_bad); return 1; }
    printf("done 1\n");
    return 0;
}
