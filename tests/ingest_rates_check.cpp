// Stand-alone host program over openwakeword_amd/csrc/owwhip_ingest.h (no HIP), for AddressSanitizer / UBSan: the table row and the
// message geometry the library itself derives for the cases of tests/ingest_rates.py (tests/test_ingest_rates_cpu.py builds and runs
// it and holds its Python mirror to these lines; it is never loaded into Python).
// Arguments: one "enc:p:q:n_taps:n_in" per case.  Prints one line per case, then the staging edge of the longest history the server
// serves (96 kHz: p / q = 6 / 1, 154 taps): the largest whole message oww_ingest accepts there and the first it refuses.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "owwhip_ingest.h"

static std::vector<float> bank(int q, int n_taps) {
    std::vector<float> t((size_t)q * n_taps);
    for (size_t i = 0; i < t.size(); ++i) t[i] = (float)(i % 7) - 3.f;
    return t;
}

static int one_row(int enc, int p, int q, int n_taps, const std::vector<float>& taps, owi::Table& t) {
    const oww_ingest_class k{enc, p, q, n_taps, n_taps ? taps.data() : nullptr};
    return owi::table_build("c", 1, &k, t, false);
}

int main(int argc, char** argv) {
    char dummy[16];
    for (int i = 1; i < argc; ++i) {
        int enc, p, q, n_taps, n_in;
        if (sscanf(argv[i], "%d:%d:%d:%d:%d", &enc, &p, &q, &n_taps, &n_in) != 5) {
            fprintf(stderr, "bad case %s\n", argv[i]);
            return 2;
        }
        const std::vector<float> taps = bank(q, n_taps);
        owi::Table t;
        int rc = one_row(enc, p, q, n_taps, taps, t);
        if (rc) {
            printf("%s table rc=%d %s\n", argv[i], rc, owp::g_err.c_str());
            continue;
        }
        const owi::ClassDev& k = t.dev[0];
        owi::ClassGeometry c;
        rc = owi::class_geometry("g", -1, k, n_in, c);
        long long n_out = -1;
        owi::Geometry g;
        const int rs = owi::single_check("s", t, dummy, n_in, n_out, g);
        printf("%s rc=%d slide=%d ntp=%d Hpad=%d xs_len=%d stage=%zu lds_bare=%zu lds_with_taps=%zu taps_in_lds=%d single_rc=%d n_out=%lld lds=%zu row=%lld\n",
               argv[i], rc, k.slide, k.ntp, k.Hpad, c.xs_len, c.stage, c.lds_bare, c.lds_with_taps, c.taps_in_lds, rs, n_out, g.lds, g.min_row_bytes);
    }
    // the staging edge at 96 kHz: whole messages are multiples of p = 6 samples
    const std::vector<float> taps = bank(1, 154);
    owi::Table t;
    if (one_row(0, 6, 1, 154, taps, t)) return 3;
    long long last = 0, first = 0, n_out = 0;
    owi::Geometry g;
    for (int n_in = 6; n_in < (1 << 20) && !first; n_in += 6) {
        if (owi::single_check("s", t, dummy, n_in, n_out, g) == 0) last = n_in;
        else first = n_in;
    }
    printf("edge96 last=%lld first=%lld %s\n", last, first, owp::g_err.c_str());
    return 0;
}
