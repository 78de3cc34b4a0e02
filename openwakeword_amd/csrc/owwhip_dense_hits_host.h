// owwhip_dense_hits_host.h -- what the host knows about the ordered hit lists of dense scoring (include/owwhip.h: oww_score_hits_layout,
// oww_score_hits, oww_score_clip_hits, oww_bank_score_hits): the geometry of the hit mask the sliding kernels write
// (owwhip_dense.h, MASK mode), the 64-bit sizes of mask, hit buffer, windows and slabs, the win_offset table, the argument checks of the
// entries, the slab plan over a column's stored hits, and a scalar statement of the ordered compaction -- mask words to list, with cap
// and total -- which dense_hits_compact_kernel implements and tests/dense_hits_check.cpp uses as the definition.  Host only and free of
// HIP, like owwhip_dense_host.h and owwhip_dense_bank_host.h, on which it builds.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "owwhip_dense_bank_host.h"

namespace owdh {

using owp::fail;

constexpr int64_t kCapMax = 1ll << 20;          // hits stored per column and call
constexpr int64_t kHitBytes = 16;               // sizeof(oww_dense_hit)

// ---- the mask: mask[col][seq][word], bit i of word k of a sequence = window 32 k + i; bits of windows >= n_win are 0.  A column's
//      words are padded to a multiple of four, so that a column starts 16-byte aligned and the compaction loads four words at a time. ----
inline int64_t words_per_seq(int64_t nw) { return (nw + 31) / 32; }
inline int64_t col_stride(int64_t B, int64_t nw) { return (B * words_per_seq(nw) + 3) / 4 * 4; }                  // words
inline uint64_t mask_bytes(int64_t n_cols, int64_t B, int64_t nw) { return (uint64_t)n_cols * (uint64_t)col_stride(B, nw) * 4u; }
// slots per column of the device's record buffer: a column has at most B x n_win hits
inline int64_t cap_eff(int64_t cap, int64_t B, int64_t nw) { return std::min<int64_t>(cap, B * nw); }
inline uint64_t hits_bytes(int64_t n_cols, int64_t cap) { return (uint64_t)n_cols * (uint64_t)cap * (uint64_t)kHitBytes; }

// ---- windows: column c holds [cap][T_c][96] floats from win_offset[c] on; win_offset[n_cols] = the total ----
inline void win_offsets(const int* T, int64_t n_cols, int64_t cap, int64_t* win_offset) {
    int64_t at = 0;
    for (int64_t c = 0; c < n_cols; ++c) { win_offset[c] = at; at += cap * (int64_t)T[c] * 96; }
    win_offset[n_cols] = at;
}
inline uint64_t windows_bytes(const int* T, int64_t n_cols, int64_t cap) {
    uint64_t rows = 0;
    for (int64_t c = 0; c < n_cols; ++c) rows += (uint64_t)T[c];
    return rows * (uint64_t)cap * (uint64_t)owd::kWindowRowBytes;
}

// ---- the slab plan over a column's stored hits: pieces [first, first + n) that cover [0, n_stored) in order, each within the budget ----
struct HitSlab { int64_t first, n; };
inline std::vector<HitSlab> slab_plan(int64_t n_stored, int64_t T, int64_t budget = owd::kSlabBytes) {
    std::vector<HitSlab> v;
    const owd::Slab sl = owd::slab(n_stored, T, budget);
    for (int64_t s = 0; s < sl.n_slabs; ++s) v.push_back(HitSlab{s * sl.windows, std::min<int64_t>(sl.windows, n_stored - s * sl.windows)});
    return v;
}

// ---- the ordered compaction, stated in scalars: the set bits of a column's words [B][wps] in (seq, word, bit) order; bit number r goes
//      to slot r while r < cap.  Returns the column's total. ----
struct Pos { int32_t seq, window; };
inline int64_t compact(const uint32_t* words, int64_t B, int64_t wps, int64_t cap, Pos* out) {
    int64_t r = 0;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t k = 0; k < wps; ++k)
            for (uint32_t bits = words[b * wps + k]; bits; bits &= bits - 1, ++r) {
                int bit = 0;
                while (!((bits >> bit) & 1u)) ++bit;
                if (r < cap) out[r] = Pos{(int32_t)b, (int32_t)(k * 32 + bit)};
            }
    return r;
}

// ---- argument checks: nothing has moved when one of them refuses ----
inline int cap_check(const char* fn, int64_t cap) {
    if (cap < 1 || cap > kCapMax) return fail(OWW_EINVAL, "%s: cap = %lld, need 1 <= cap <= %lld", fn, (long long)cap, (long long)kCapMax);
    return 0;
}
inline int layout_check(const char* fn, int64_t cap, const void* win_offset) {
    if (!win_offset) return fail(OWW_EINVAL, "%s: null win_offset", fn);
    return cap_check(fn, cap);
}
// the outputs every entry shares, and the sizes of what the call allocates.  T[c]: the window length of column c's head.
inline int outputs_check(const char* fn, int64_t cap, const void* hits, const void* n_stored, const void* n_total, const void* windows,
                         int windows_on_device) {
    if (int rc = cap_check(fn, cap)) return rc;
    if (!hits || !n_stored || !n_total) return fail(OWW_EINVAL, "%s: hits, n_stored and n_total are required", fn);
    if (windows && windows_on_device && (reinterpret_cast<uintptr_t>(windows) & 15)) return fail(OWW_EINVAL, "%s: a device windows buffer must be 16-byte aligned", fn);
    return 0;
}
inline int sizes_check(const char* fn, int64_t B, int64_t n_rows, int64_t t_max, int64_t n_cols, int64_t cap) {
    const int64_t nw = owd::n_win(n_rows, t_max);
    const uint64_t fb = owd::feats_bytes(B, n_rows);
    if (fb > owd::kMaxBytes || (uint64_t)B * (uint64_t)n_rows > (uint64_t)INT64_MAX / 1024)
        return fail(OWW_ENOMEM, "%s: %llu bytes of features do not fit", fn, (unsigned long long)fb);
    const uint64_t mb = mask_bytes(n_cols, B, nw), hb = hits_bytes(n_cols, cap_eff(cap, B, nw));
    if (mb > owd::kMaxBytes || hb > owd::kMaxBytes)
        return fail(OWW_ENOMEM, "%s: %llu bytes of hit mask and %llu bytes of hit records do not fit", fn, (unsigned long long)mb, (unsigned long long)hb);
    if (B * owd::tiles_per_seq(nw, owd::kWavesSmall) > owd::kMaxGrid)
        return fail(OWW_ENOMEM, "%s: %lld sequences x %lld tiles exceed one launch (%llu bytes of features); score in chunks", fn, (long long)B,
                    (long long)owd::tiles_per_seq(nw, owd::kWavesSmall), (unsigned long long)fb);
    return 0;
}
inline int features_check(const char* fn, const void* feats, int feats_on_device, int64_t B, int64_t n_rows, int64_t t_max, int64_t n_cols, int64_t cap,
                          const void* hits, const void* n_stored, const void* n_total, const void* windows, int windows_on_device) {
    if (!feats || B < 1) return fail(OWW_EINVAL, "%s: bad argument (B = %lld, null features)", fn, (long long)B);
    if (int rc = outputs_check(fn, cap, hits, n_stored, n_total, windows, windows_on_device)) return rc;
    if (int rc = owd::rows_check(fn, feats, feats_on_device, n_rows, t_max)) return rc;
    return sizes_check(fn, B, n_rows, t_max, n_cols, cap);
}
inline int clips_check(const char* fn, const void* pcm, int64_t B, int64_t n, int64_t n_streams, int64_t t_max, int64_t n_cols, int64_t cap,
                       const void* hits, const void* n_stored, const void* n_total, const void* windows, int windows_on_device) {
    if (!pcm || B < 1 || B > n_streams) return fail(OWW_EINVAL, "%s: bad argument (B = %lld, need 1 <= B <= %lld)", fn, (long long)B, (long long)n_streams);
    if (int rc = outputs_check(fn, cap, hits, n_stored, n_total, windows, windows_on_device)) return rc;
    const int64_t rows = owd::clip_rows(n);
    if (rows < 1) return fail(OWW_EINVAL, "%s: %lld samples give no embedding (one needs 12,512)", fn, (long long)n);
    if (int rc = owd::shape_check(fn, rows, t_max)) return rc;
    return sizes_check(fn, B, rows, t_max, n_cols, cap);
}
// the bank entry: a NaN threshold is refused, as oww_bank_score_stats refuses it
inline int bank_thresholds_check(const char* fn, const float* thresholds, int64_t n_ids) {
    if (thresholds)
        for (int64_t i = 0; i < n_ids; ++i)
            if (std::isnan(thresholds[i])) return fail(OWW_EINVAL, "%s: threshold %lld is NaN", fn, (long long)i);
    return 0;
}

}  // namespace owdh
