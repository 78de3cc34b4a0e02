// Stand-alone host program over openwakeword_amd/csrc/owwhip_ingest.h (no HIP): the class table, every argument check of both ingest
// forms, the message geometry that sizes a launch's LDS and the ingest part of the state fingerprint, for AddressSanitizer / UBSan (tests/test_ingest_mixed_cpu.py builds and runs it; it is never loaded into Python).
// Reads nothing; prints one line per case: name, return code, and what the case produced.
#include <cstdio>
#include <vector>

#include "owwhip_ingest.h"

static std::vector<float> bank(int q, int n_taps) {
    std::vector<float> t((size_t)q * n_taps);
    for (size_t i = 0; i < t.size(); ++i) t[i] = (float)(i % 7) - 3.f;
    return t;
}

static const char* msg(int rc) { return rc ? owp::g_err.c_str() : "-"; }

// the single form's one-row table, as oww_ingest_configure builds it
static int one_row(int enc, int p, int q, int n_taps, const float* taps, owi::Table& t) {
    const oww_ingest_class k{enc, p, q, n_taps, taps};
    return owi::table_build("c", 1, &k, t, false);
}

// the two hashing formulas as the handle had them before owi::fingerprint: the single form from its scalar fields and its own padded
// bank, the class form from the table
static uint64_t old_single_fp(uint64_t fp, int enc, int p, int q, int n_taps, const float* taps) {
    const int ntp = (n_taps + 3) / 4 * 4;
    std::vector<float> padded((size_t)q * ntp, 0.f);
    for (int r = 0; r < q && n_taps; ++r) memcpy(&padded[(size_t)r * ntp], taps + (size_t)r * n_taps, n_taps * sizeof(float));
    const int32_t ig[4] = {enc, p, q, n_taps};
    fp = owp::fp_mix(fp, ig, sizeof ig);
    return owp::fp_mix(fp, padded.data(), padded.size() * sizeof(float));
}
static uint64_t old_classes_fp(uint64_t fp, const owi::Table& t) {
    const int32_t tag[2] = {-1, (int32_t)t.dev.size()};
    fp = owp::fp_mix(fp, tag, sizeof tag);
    fp = owp::fp_mix(fp, t.dev.data(), t.dev.size() * sizeof(owi::ClassDev));
    return owp::fp_mix(fp, t.banks.data(), t.banks.size() * sizeof(float));
}

int main() {
    // the server's full table: 11 rates as PCM16 with resample.design's (p, q, n_taps), G.711 at 8 kHz
    const int fmt[13][4] = {{0, 1, 2, 26},   {0, 441, 640, 26}, {0, 3, 4, 26},   {0, 1, 1, 0},     {0, 441, 320, 36}, {0, 3, 2, 40}, {0, 2, 1, 52},
                            {0, 441, 160, 70}, {0, 3, 1, 78},   {0, 441, 80, 140}, {0, 6, 1, 154}, {1, 1, 2, 26},     {2, 1, 2, 26}};
    std::vector<std::vector<float>> banks;
    std::vector<oww_ingest_class> cls;
    for (const auto& f : fmt) {
        banks.push_back(bank(f[2], f[3]));
        cls.push_back(oww_ingest_class{f[0], f[1], f[2], f[3], f[3] ? banks.back().data() : nullptr});
    }
    owi::Table t;
    int rc = owi::table_build("t", (int)cls.size(), cls.data(), t);
    unsigned long long sum = 0;
    for (float v : t.banks) sum = sum * 31 + (unsigned long long)(long long)(v + 3.f);
    printf("full rc=%d classes=%zu bank_floats=%zu Hpad_max=%d last_off=%d last_slide=%d sum=%llu\n", rc, t.dev.size(), t.banks.size(), t.Hpad_max,
           t.dev.empty() ? -1 : t.dev.back().taps_off, t.dev.empty() ? -1 : t.dev.back().slide, sum);
    // rows of the padded banks: n_taps = 26 -> ntp = 28, the two pad taps zero
    printf("pad ntp=%d tail=%g,%g first=%g\n", t.dev[0].ntp, t.banks[26], t.banks[27], t.banks[28]);

    owi::Geometry g;
    char dummy[16];
    rc = owi::mixed_check("m", t, dummy, 15360, 1280, g);
    printf("frame rc=%d lds=%zu min_row=%lld %s\n", rc, g.lds, g.min_row_bytes, msg(rc));
    rc = owi::mixed_check("m", t, dummy, 15344, 1280, g);
    printf("row_small rc=%d %s\n", rc, msg(rc));
    rc = owi::mixed_check("m", t, dummy, 15368, 1280, g);
    printf("row_odd rc=%d %s\n", rc, msg(rc));
    rc = owi::mixed_check("m", t, dummy, 15360, 100, g);
    printf("not_whole rc=%d %s\n", rc, msg(rc));
    rc = owi::mixed_check("m", t, dummy, 1 << 20, 5120, g);
    printf("lds rc=%d %s\n", rc, msg(rc));
    rc = owi::mixed_check("m", t, nullptr, 15360, 1280, g);
    printf("null_in rc=%d %s\n", rc, msg(rc));
    rc = owi::mixed_check("m", t, dummy, 15360, 0, g);
    printf("n_out0 rc=%d %s\n", rc, msg(rc));
    rc = owi::mixed_check("m", t, dummy, 1ll << 40, (1 << 24) + 1, g);
    printf("n_out_big rc=%d %s\n", rc, msg(rc));

    // refused tables leave the target untouched
    owi::Table keep = t;
    std::vector<oww_ingest_class> many(17, cls[0]);
    rc = owi::table_build("t", 17, many.data(), t);
    printf("seventeen rc=%d kept=%d %s\n", rc, (int)(t.dev.size() == keep.dev.size()), msg(rc));
    rc = owi::table_build("t", 0, many.data(), t);
    printf("zero rc=%d %s\n", rc, msg(rc));
    rc = owi::table_build("t", 1, nullptr, t);
    printf("null rc=%d %s\n", rc, msg(rc));
    const int bad[6][4] = {{7, 1, 2, 26}, {1, 1, 2, 25}, {1, 2, 1, 0}, {1, 0, 2, 26}, {1, 1, 65537, 26}, {1, 1, 2, 4098}};
    for (int i = 0; i < 6; ++i) {
        many[3] = oww_ingest_class{bad[i][0], bad[i][1], bad[i][2], bad[i][3], banks[0].data()};
        rc = owi::table_build("t", 4, many.data(), t);
        printf("bad%d rc=%d kept=%d %s\n", i, rc, (int)(t.dev.size() == keep.dev.size()), msg(rc));
    }
    many[3] = oww_ingest_class{1, 1, 2, 26, nullptr};
    rc = owi::table_build("t", 4, many.data(), t);
    printf("null_taps rc=%d %s\n", rc, msg(rc));
    // decode only everywhere: no history, one float of bank so that the device buffer exists
    std::vector<oww_ingest_class> dec(3, oww_ingest_class{2, 1, 1, 0, nullptr});
    owi::Table d;
    rc = owi::table_build("t", 3, dec.data(), d);
    printf("decode_only rc=%d Hpad_max=%d bank_floats=%zu\n", rc, d.Hpad_max, d.banks.size());

    const int32_t ids[3] = {0, 5, 36};
    const uint8_t c_ok[3] = {0, 12, 3}, c_bad[3] = {0, 13, 3};
    rc = owi::assign_check("a", t, 37, ids, 3, c_ok);
    printf("assign_ok rc=%d\n", rc);
    rc = owi::assign_check("a", t, 37, ids, 3, c_bad);
    printf("assign_class rc=%d %s\n", rc, msg(rc));
    rc = owi::assign_check("a", t, 36, ids, 3, c_ok);
    printf("assign_stream rc=%d %s\n", rc, msg(rc));
    rc = owi::assign_check("a", t, 37, nullptr, 3, c_ok);
    printf("assign_null rc=%d %s\n", rc, msg(rc));
    rc = owi::assign_check("a", t, 37, nullptr, 0, nullptr);
    printf("assign_none rc=%d\n", rc);

    // the single form: a table of one row whose messages name no class, and single_check on it
    owi::Table u, w, big;
    rc = one_row(1, 1, 2, 26, banks[0].data(), u);
    printf("one_row rc=%d classes=%zu bank_floats=%zu Hpad_max=%d ntp=%d slide=%d\n", rc, u.dev.size(), u.banks.size(), u.Hpad_max, u.dev[0].ntp, u.dev[0].slide);
    const int bad1[5][4] = {{7, 1, 2, 26}, {1, 1, 2, 25}, {1, 2, 1, 0}, {1, 0, 2, 26}, {1, 1, 2, 26}};
    for (int i = 0; i < 5; ++i) {
        rc = one_row(bad1[i][0], bad1[i][1], bad1[i][2], bad1[i][3], i == 4 ? nullptr : banks[0].data(), u);
        printf("one_bad%d rc=%d kept=%d %s\n", i, rc, (int)(u.dev.size() == 1 && u.dev[0].n_taps == 26), msg(rc));
    }
    long long n_out = -1;
    owi::Geometry sg;
    rc = owi::single_check("s", u, dummy, 640, n_out, sg);
    printf("s_ulaw rc=%d n_out=%lld lds=%zu xs_len=%d taps_in_lds=%d row=%lld %s\n", rc, n_out, sg.lds, sg.xs_len, sg.taps_in_lds, sg.min_row_bytes, msg(rc));
    rc = owi::single_check("s", u, dummy, 0, n_out, sg);
    printf("s_zero rc=%d n_out=%lld %s\n", rc, n_out, msg(rc));
    rc = owi::single_check("s", u, dummy, 30000, n_out, sg);
    printf("s_lds rc=%d n_out=%lld %s\n", rc, n_out, msg(rc));
    rc = owi::single_check("s", u, nullptr, 640, n_out, sg);
    printf("s_null rc=%d %s\n", rc, msg(rc));
    rc = owi::single_check("s", u, dummy, 1 << 24, n_out, sg);                // n_out = 2^25: refused before any LDS arithmetic
    printf("s_n_out_big rc=%d %s\n", rc, msg(rc));
    rc = one_row(0, 441, 160, 70, banks[7].data(), w);
    rc = rc ? rc : owi::single_check("s", w, dummy, 100, n_out, sg);
    printf("s_not_whole rc=%d %s\n", rc, msg(rc));
    // a bank that does not fit LDS (16001 Hz: p = 16001, q = 16000, 16000 x 28 floats): read from global memory, the LDS need excludes it
    const std::vector<float> bank16001 = bank(16000, 26);
    rc = one_row(0, 16001, 16000, 26, bank16001.data(), big);
    rc = rc ? rc : owi::single_check("s", big, dummy, 16001, n_out, sg);
    printf("s_big_bank rc=%d n_out=%lld lds=%zu xs_len=%d taps_in_lds=%d bank_floats=%zu %s\n", rc, n_out, sg.lds, sg.xs_len, sg.taps_in_lds, big.banks.size(), msg(rc));

    // the fingerprint against the two formulas it replaces
    const uint64_t seed = 1469598103934665603ull;
    owi::Table a8;
    one_row(2, 1, 1, 0, nullptr, a8);                                        // decode-only A-law: the placeholder float is not hashed
    one_row(1, 1, 2, 26, banks[0].data(), u);
    printf("fp_ulaw8k equal=%d\n", (int)(owi::fingerprint(seed, true, false, u) == old_single_fp(seed, 1, 1, 2, 26, banks[0].data())));
    printf("fp_pcm44k equal=%d\n", (int)(owi::fingerprint(seed, true, false, w) == old_single_fp(seed, 0, 441, 160, 70, banks[7].data())));
    printf("fp_alaw_decode equal=%d placeholder=%zu\n", (int)(owi::fingerprint(seed, true, false, a8) == old_single_fp(seed, 2, 1, 1, 0, nullptr)), a8.banks.size());
    printf("fp_full equal=%d\n", (int)(owi::fingerprint(seed, true, true, keep) == old_classes_fp(seed, keep)));
    printf("fp_decode_table equal=%d\n", (int)(owi::fingerprint(seed, true, true, d) == old_classes_fp(seed, d)));
    printf("fp_none equal=%d\n", (int)(owi::fingerprint(seed, false, false, owi::Table()) == seed));
    const oww_ingest_class k8{1, 1, 2, 26, banks[0].data()};
    owi::Table one_class;
    owi::table_build("t", 1, &k8, one_class);
    printf("fp_single_vs_one_class differ=%d same_rows=%d\n", (int)(owi::fingerprint(seed, true, false, u) != owi::fingerprint(seed, true, true, one_class)),
           (int)(memcmp(u.dev.data(), one_class.dev.data(), sizeof(owi::ClassDev)) == 0 && u.banks == one_class.banks));
    return 0;
}
