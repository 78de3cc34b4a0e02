// Stand-alone host program over openwakeword_amd/csrc/owwhip_ingest.h (no HIP): the class table and every argument check of the ingest
// classes, for AddressSanitizer / UBSan (tests/test_ingest_mixed_cpu.py builds and runs it; it is never loaded into Python).
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
    return 0;
}
