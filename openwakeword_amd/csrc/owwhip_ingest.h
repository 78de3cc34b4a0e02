// owwhip_ingest.h -- the host side of the ingest classes (oww_ingest_configure_classes / oww_ingest_mixed): per-class argument checks,
// the class table with its padded banks back to back, and the per-call geometry checks (whole n_in per class, row_bytes, the LDS
// rule).  Host only and free of HIP, like owwhip_pack.h: owwhip.hip includes it for the library, and tests/ingest_classes_check.cpp
// includes it alone under AddressSanitizer / UBSan.  The device reads what `Table::dev` holds as owk::IngestClass rows.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "owwhip.h"
#include "owwhip_pack.h"

namespace owi {

using owp::fail;

constexpr int kTile = 256 * 8;                  // = owk::IG_TILE (outputs per tile; its int16 staging is kTile / 2 floats of LDS)
constexpr size_t kLdsStage = 96 * 1024;         // history + message as floats: what one workgroup stages at most
constexpr size_t kLdsWithTaps = 150 * 1024;     // ... and with the bank behind it

struct ClassDev { int32_t enc, p, q, n_taps, ntp, Hpad, taps_off, slide; };   // = owk::IngestClass

struct Table {
    std::vector<ClassDev> dev;                  // one row per class
    std::vector<float> banks;                   // every class's [q][ntp] bank, zero padded rows, back to back (at least one float)
    int Hpad_max = 0;
};

// what oww_ingest_configure checks, for one class; `fn` and `idx` (< 0: no class index) only shape the message
inline int class_check(const char* fn, int idx, int32_t encoding, int32_t p, int32_t q, const float* taps, int32_t n_taps) {
    char who[32] = "";
    if (idx >= 0) snprintf(who, sizeof who, "class %d: ", idx);
    if (encoding != OWW_ENC_PCM16 && encoding != OWW_ENC_ULAW && encoding != OWW_ENC_ALAW)
        return fail(OWW_EINVAL, "%s: %sunknown encoding %d (OWW_ENC_PCM16 = 0, OWW_ENC_ULAW = 1, OWW_ENC_ALAW = 2)", fn, who, encoding);
    if (n_taps == 0) {
        if (p != 1 || q != 1) return fail(OWW_EINVAL, "%s: %sn_taps = 0 (decode only) needs p = q = 1, got p=%d q=%d", fn, who, p, q);
    } else {
        if (p < 1 || q < 1 || n_taps < 2 || (n_taps & 1) || n_taps > 4096 || q > 65536)
            return fail(OWW_EINVAL, "%s: %sbad argument (p=%d q=%d n_taps=%d)", fn, who, p, q, n_taps);
        if (!taps) return fail(OWW_EINVAL, "%s: %snull argument: taps", fn, who);
    }
    return 0;
}

// the table of n classes; `t` is written only when every class passes
inline int table_build(const char* fn, int32_t n, const oww_ingest_class* classes, Table& t) {
    if (n < 1 || n > OWW_INGEST_MAX_CLASSES) return fail(OWW_EINVAL, "%s: n_classes=%d outside [1,%d]", fn, n, OWW_INGEST_MAX_CLASSES);
    if (!classes) return fail(OWW_EINVAL, "%s: null argument: classes", fn);
    for (int c = 0; c < n; ++c)
        if (int rc = class_check(fn, c, classes[c].encoding, classes[c].p, classes[c].q, classes[c].taps, classes[c].n_taps)) return rc;
    Table b;
    for (int c = 0; c < n; ++c) {
        const oww_ingest_class& k = classes[c];
        const int ntp = (k.n_taps + 3) / 4 * 4, Hpad = k.n_taps ? (k.n_taps - 1 + 7) / 8 * 8 : 0;
        const size_t at = b.banks.size();
        if (at + (size_t)k.q * ntp > (size_t)INT32_MAX) return fail(OWW_EINVAL, "%s: the banks of %d classes exceed 2^31 floats", fn, n);
        b.banks.resize(at + (size_t)k.q * ntp, 0.f);
        for (int r = 0; r < k.q && k.n_taps; ++r) memcpy(&b.banks[at + (size_t)r * ntp], k.taps + (size_t)r * k.n_taps, k.n_taps * sizeof(float));
        const int slide = k.n_taps && k.p == 1 && (k.q == 1 || k.q == 2 || k.q == 4 || k.q == 8);
        b.dev.push_back(ClassDev{k.encoding, k.p, k.q, k.n_taps, ntp, Hpad, (int32_t)at, slide});
        if (Hpad > b.Hpad_max) b.Hpad_max = Hpad;
    }
    if (b.banks.empty()) b.banks.push_back(0.f);
    t = std::move(b);
    return 0;
}

struct Geometry { size_t lds = 0; long long min_row_bytes = 0; };

// one oww_ingest_mixed call against the table: nothing has moved when this refuses
inline int mixed_check(const char* fn, const Table& t, const void* in, long long row_bytes, long long n_out, Geometry& g) {
    if (!in) return fail(OWW_EINVAL, "%s: null argument: in", fn);
    if (n_out < 1 || n_out > (1 << 24)) return fail(OWW_EINVAL, "%s: bad argument (n_out=%lld; at most 2^24 samples per message)", fn, n_out);
    if (row_bytes < 16 || row_bytes % 16) return fail(OWW_EINVAL, "%s: row_bytes = %lld must be a positive multiple of 16", fn, row_bytes);
    Geometry b;
    for (size_t c = 0; c < t.dev.size(); ++c) {
        const ClassDev& k = t.dev[c];
        if ((n_out * k.p) % k.q)
            return fail(OWW_EINVAL, "%s: class %zu has no whole message for n_out = %lld: n_out * p = %lld * %d is no multiple of q = %d", fn, c, n_out, n_out, k.p, k.q);
        const long long n_in = n_out * k.p / k.q, bytes = n_in * (k.enc == OWW_ENC_PCM16 ? 2 : 1);
        if (n_in < 1 || n_in > (1 << 24)) return fail(OWW_EINVAL, "%s: class %zu: n_in = %lld outside [1, 2^24]", fn, c, n_in);
        const int H = k.n_taps ? k.n_taps - 1 : 0, Hoff = (H + 3) / 4 * 4;
        const size_t xs_len = (size_t)(Hoff + n_in + 8 + 3) / 4 * 4;
        const size_t lds_x = xs_len * sizeof(float), lds_y = (size_t)kTile * sizeof(int16_t), lds_t = (size_t)k.q * k.ntp * sizeof(float);
        if (lds_x > kLdsStage)
            return fail(OWW_EINVAL, "%s: class %zu: a message of n_in = %lld samples behind a history of %d needs %zu bytes of LDS, the one-workgroup-per-stream "
                                    "kernel stages at most %zu: send shorter messages", fn, c, n_in, H, lds_x, kLdsStage);
        const size_t need = lds_x + lds_y + (k.n_taps && lds_x + lds_y + lds_t <= kLdsWithTaps ? lds_t : 0);
        if (need > b.lds) b.lds = need;
        if (bytes > b.min_row_bytes) b.min_row_bytes = bytes;
    }
    if (row_bytes < b.min_row_bytes)
        return fail(OWW_EINVAL, "%s: row_bytes = %lld is less than the largest configured class's message of %lld bytes", fn, row_bytes, b.min_row_bytes);
    g = b;
    return 0;
}

// oww_ingest_assign's lists
inline int assign_check(const char* fn, const Table& t, int S, const int32_t* stream_ids, int32_t n, const uint8_t* class_ids) {
    if (n < 0 || (n > 0 && (!stream_ids || !class_ids))) return fail(OWW_EINVAL, "%s: bad argument (n=%d, null list)", fn, n);
    for (int i = 0; i < n; ++i) {
        if (stream_ids[i] < 0 || stream_ids[i] >= S) return fail(OWW_EINVAL, "%s: stream id %d out of range", fn, stream_ids[i]);
        if (class_ids[i] >= t.dev.size()) return fail(OWW_EINVAL, "%s: unknown class %d (the handle has %zu)", fn, (int)class_ids[i], t.dev.size());
    }
    return 0;
}

}  // namespace owi
