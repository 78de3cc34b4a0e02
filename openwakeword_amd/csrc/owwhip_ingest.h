// owwhip_ingest.h -- everything the host knows about ingest arithmetic, for the single form (oww_ingest_configure / oww_ingest) and the
// class form (oww_ingest_configure_classes / oww_ingest_mixed) alike: the bank padder, the per-class argument checks, the class table
// with its padded banks back to back (the single form is a table of one row), the per-class message geometry that sizes a launch's
// dynamic LDS, the per-call checks of both forms on top of it, and the ingest part of the state fingerprint.  Host only and free of
// HIP, like owwhip_pack.h: owwhip.hip includes it for the library, where it keeps the buffers and launches, and
// tests/ingest_classes_check.cpp includes it alone under AddressSanitizer / UBSan.  The device reads what `Table::dev` holds as
// owk::IngestClass rows.
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

// the bank as the kernels read it, appended to `out`: [q][n_taps] becomes [q][ntp], ntp = n_taps rounded up to 4, zero filled
inline void bank_pad(const float* taps, int q, int n_taps, std::vector<float>& out) {
    const int ntp = (n_taps + 3) / 4 * 4;
    const size_t at = out.size();
    out.resize(at + (size_t)q * ntp, 0.f);
    for (int r = 0; r < q && n_taps; ++r) memcpy(&out[at + (size_t)r * ntp], taps + (size_t)r * n_taps, n_taps * sizeof(float));
}

struct Who { char s[32] = ""; explicit Who(int idx) { if (idx >= 0) snprintf(s, sizeof s, "class %d: ", idx); } };   // idx < 0: no class index

// one class's arguments; `fn` and `idx` only shape the message
inline int class_check(const char* fn, int idx, int32_t encoding, int32_t p, int32_t q, const float* taps, int32_t n_taps) {
    const Who who(idx);
    if (encoding != OWW_ENC_PCM16 && encoding != OWW_ENC_ULAW && encoding != OWW_ENC_ALAW)
        return fail(OWW_EINVAL, "%s: %sunknown encoding %d (OWW_ENC_PCM16 = 0, OWW_ENC_ULAW = 1, OWW_ENC_ALAW = 2)", fn, who.s, encoding);
    if (n_taps == 0) {
        if (p != 1 || q != 1) return fail(OWW_EINVAL, "%s: %sn_taps = 0 (decode only) needs p = q = 1, got p=%d q=%d", fn, who.s, p, q);
    } else {
        if (p < 1 || q < 1 || n_taps < 2 || (n_taps & 1) || n_taps > 4096 || q > 65536)
            return fail(OWW_EINVAL, "%s: %sbad argument (p=%d q=%d n_taps=%d)", fn, who.s, p, q, n_taps);
        if (!taps) return fail(OWW_EINVAL, "%s: %snull argument: taps", fn, who.s);
    }
    return 0;
}

// the table of n classes; `t` is written only when every class passes.  numbered = false: the single form's one row, whose messages
// name no class
inline int table_build(const char* fn, int32_t n, const oww_ingest_class* classes, Table& t, bool numbered = true) {
    if (n < 1 || n > OWW_INGEST_MAX_CLASSES) return fail(OWW_EINVAL, "%s: n_classes=%d outside [1,%d]", fn, n, OWW_INGEST_MAX_CLASSES);
    if (!classes) return fail(OWW_EINVAL, "%s: null argument: classes", fn);
    for (int c = 0; c < n; ++c)
        if (int rc = class_check(fn, numbered ? c : -1, classes[c].encoding, classes[c].p, classes[c].q, classes[c].taps, classes[c].n_taps)) return rc;
    Table b;
    for (int c = 0; c < n; ++c) {
        const oww_ingest_class& k = classes[c];
        const int ntp = (k.n_taps + 3) / 4 * 4, Hpad = k.n_taps ? (k.n_taps - 1 + 7) / 8 * 8 : 0;
        const size_t at = b.banks.size();
        if (at + (size_t)k.q * ntp > (size_t)INT32_MAX) return fail(OWW_EINVAL, "%s: the banks of %d classes exceed 2^31 floats", fn, n);
        bank_pad(k.taps, k.q, k.n_taps, b.banks);
        const int slide = k.n_taps && k.p == 1 && (k.q == 1 || k.q == 2 || k.q == 4 || k.q == 8);
        b.dev.push_back(ClassDev{k.encoding, k.p, k.q, k.n_taps, ntp, Hpad, (int32_t)at, slide});
        if (Hpad > b.Hpad_max) b.Hpad_max = Hpad;
    }
    if (b.banks.empty()) b.banks.push_back(0.f);
    t = std::move(b);
    return 0;
}

// one class's message of n_in samples in one workgroup's LDS: history + message as floats (`stage` bytes, xs_len floats), the int16
// output tile, and the class's bank behind them where all three fit kLdsWithTaps
struct ClassGeometry {
    int xs_len = 0, taps_in_lds = 0;
    size_t stage = 0, lds_bare = 0, lds_with_taps = 0;
    size_t lds() const { return taps_in_lds ? lds_with_taps : lds_bare; }   // the dynamic LDS of a launch that serves this class
};

// 1 <= n_in <= 2^31; refuses a message that one workgroup cannot stage
inline int class_geometry(const char* fn, int idx, const ClassDev& k, long long n_in, ClassGeometry& g) {
    const int H = k.n_taps ? k.n_taps - 1 : 0, Hoff = (H + 3) / 4 * 4;
    const size_t xs_len = (size_t)(Hoff + n_in + 8 + 3) / 4 * 4;   // (+ 8: what the zero-padded taps, and the sliding form's look-ahead quad, read on)
    g.stage = xs_len * sizeof(float);
    if (g.stage > kLdsStage)
        return fail(OWW_EINVAL, "%s: %sa message of n_in = %lld samples behind a history of %d needs %zu bytes of LDS, the one-workgroup-per-stream "
                                "kernel stages at most %zu: send shorter messages", fn, Who(idx).s, n_in, H, g.stage, kLdsStage);
    g.xs_len = (int)xs_len;
    g.lds_bare = g.stage + (size_t)kTile * sizeof(int16_t);
    g.lds_with_taps = g.lds_bare + (size_t)k.q * k.ntp * sizeof(float);
    g.taps_in_lds = k.n_taps && g.lds_with_taps <= kLdsWithTaps;
    return 0;
}

// what a launch needs to know of a checked message: `lds` its dynamic LDS, min_row_bytes the class form's widest message, xs_len and
// taps_in_lds the single form's row (its kernel takes them as parameters; the class kernel works them out per stream)
struct Geometry { size_t lds = 0; long long min_row_bytes = 0; int xs_len = 0, taps_in_lds = 0; };

// one oww_ingest / oww_step_ingest call against the single form's one-row table: nothing has moved when this refuses
inline int single_check(const char* fn, const Table& t, const void* in, int32_t n_in, long long& n_out, Geometry& g) {
    const ClassDev& k = t.dev[0];
    if (!in) return fail(OWW_EINVAL, "%s: null argument: in", fn);
    if (n_in < 1) return fail(OWW_EINVAL, "%s: bad argument (n_in=%d)", fn, n_in);
    if (((long long)n_in * k.q) % k.p)
        return fail(OWW_EINVAL, "%s: a message must hold a whole number of output samples: n_in * q = %d * %d is no multiple of p = %d", fn, n_in, k.q, k.p);
    const long long n = (long long)n_in * k.q / k.p;
    if (n > (1 << 24)) return fail(OWW_EINVAL, "%s: n_out = %lld is beyond 2^24 samples per message", fn, n);
    ClassGeometry c;
    if (int rc = class_geometry(fn, -1, k, n_in, c)) return rc;
    n_out = n;
    g = Geometry{c.lds(), (long long)n_in * (k.enc == OWW_ENC_PCM16 ? 2 : 1), c.xs_len, c.taps_in_lds};
    return 0;
}

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
        ClassGeometry cg;
        if (int rc = class_geometry(fn, (int)c, k, n_in, cg)) return rc;
        if (cg.lds() > b.lds) b.lds = cg.lds();
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

// the ingest part of the state fingerprint: what a record's history (and class word) means.  A handle that never configured ingest
// hashes nothing; the single form hashes {enc, p, q, n_taps} and its padded bank (decode only: no float -- the table's placeholder
// is not a bank); the class form a tag no single configuration can have, every row and every bank.
inline uint64_t fingerprint(uint64_t fp, bool ready, bool mixed, const Table& t) {
    if (!ready) return fp;
    if (mixed) {
        const int32_t tag[2] = {-1, (int32_t)t.dev.size()};                 // (no single configuration has encoding -1)
        fp = owp::fp_mix(fp, tag, sizeof tag);
        fp = owp::fp_mix(fp, t.dev.data(), t.dev.size() * sizeof(ClassDev));
        return owp::fp_mix(fp, t.banks.data(), t.banks.size() * sizeof(float));
    }
    const ClassDev& k = t.dev[0];
    const int32_t ig[4] = {k.enc, k.p, k.q, k.n_taps};
    fp = owp::fp_mix(fp, ig, sizeof ig);
    return owp::fp_mix(fp, t.banks.data(), (size_t)k.q * k.ntp * sizeof(float));
}

}  // namespace owi
