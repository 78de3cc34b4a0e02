// owwhip_dense_bank_host.h -- what the host knows about dense scoring over the head bank (include/owwhip.h: oww_bank_score_shape,
// oww_bank_score_features, oww_bank_score_stats): the slice plan of heads_dense_bank_kernel (owwhip_dense.h) -- how many heads one
// workgroup walks on the rows it staged, the grid, which block scores which (tile, heads) -- the staged row a k-step of a head reads,
// the order-preserving key of the statistics, the 64-bit sizes and the argument checks of the three entries.  Host only and free of HIP,
// like owwhip_dense_host.h, on which it builds: owwhip.hip includes it for the library, tests/dense_bank_check.cpp includes it alone
// under AddressSanitizer / UBSan.  The functions the kernel shares with the host are marked for both sides (OWD_HD).
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "owwhip_dense_host.h"

namespace owd {

// ---- the slice plan.  One launch covers every listed narrow head: the grid is (sequence x tile) x head slices, a slice = hpw
//      consecutive heads of the list.  A workgroup stages its tile's rows once and walks the heads of its slice, so hpw is what
//      amortises the staging (a tile's rows are 104 KB of features at t_s = 16, a head streams 384 KB of weights and runs 48 k-steps:
//      at hpw = 8 staging is a few per cent of a workgroup's time) -- and what shrinks the grid: a short corpus (30 tiles for ten
//      minutes) fills the chip only when the heads spread over workgroups.  hpw is therefore the largest value up to kBankHpwMax that
//      still leaves kBankTargetGrid workgroups (four per CU), and never so small that the grid would exceed one launch.  Blocks are
//      numbered slice-major (block = slice x tiles + tile): the workgroups in flight at one time walk the same few heads, whose
//      weights they then share in L2. ----
constexpr int kBankHpwMax = 8;
constexpr int64_t kBankTargetGrid = 1024;
struct BankPlan {
    int hpw = 0;                   // heads per workgroup; 0 = the plan refuses (rows that fit no tile, tiles beyond one launch): fallback
    int64_t seq_tiles = 0, tiles = 0, slices = 0, grid = 0;      // tiles per sequence, B x seq_tiles, head slices, tiles x slices
    Geometry geo;                  // owd::geometry(1, t_s)
};
inline BankPlan bank_plan(int64_t n_heads, int64_t B, int64_t nw, int64_t t_s, int64_t hpw_forced = 0) {
    BankPlan p;
    p.geo = geometry(1, t_s);
    if (n_heads < 1 || B < 1 || nw < 1 || !p.geo.slots) return p;
    p.seq_tiles = tiles_per_seq(nw, p.geo.waves);
    if (p.seq_tiles > kMaxGrid / B) return p;
    p.tiles = B * p.seq_tiles;
    int64_t hpw = hpw_forced > 0 ? hpw_forced : std::max<int64_t>(1, std::min<int64_t>(kBankHpwMax, n_heads * p.tiles / kBankTargetGrid));
    hpw = std::min(hpw, n_heads);
    const int64_t max_slices = kMaxGrid / p.tiles;                           // >= 1
    hpw = std::max(hpw, (n_heads + max_slices - 1) / max_slices);            // the grid stays within one launch
    p.hpw = (int)hpw;
    p.slices = (n_heads + hpw - 1) / hpw;
    p.grid = p.tiles * p.slices;
    return p;
}
// OWW_DENSE_BANK_HPW (A/B aid, and the tests' handle on the slice edges): heads per workgroup; unset, empty or < 1 = the plan's own
inline int64_t bank_hpw_env() {
    const char* e = getenv("OWW_DENSE_BANK_HPW");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (int64_t)std::min<long long>(v, INT32_MAX) : 0;
}
// block -> (slice, tile), slice -> heads [first, first + count) of the list
OWD_HD int bank_block_slice(int block, int tiles) { return block / tiles; }
OWD_HD int bank_block_tile(int block, int tiles) { return block % tiles; }
OWD_HD int bank_slice_first(int slice, int hpw) { return slice * hpw; }
OWD_HD int bank_slice_count(int slice, int hpw, int n_heads) { const int left = n_heads - slice * hpw; return left < hpw ? left : hpw; }

// ---- the staged row the B operand of k-step ks comes from: a tile stages rows [w0 + t_max - t_s, .. + 32 waves + t_s - 1) for t_s =
//      the largest T of the launch, and a head of length T reads its own last T rows of every window: position pos of tile t of wave
//      `wave` reads staged row 16 (2 wave + t) + pos + (t_s - T) + ks / 3  (<= 32 waves + t_s - 2, the last staged row) ----
OWD_HD int bank_staged_row(int wave, int t, int pos, int t_s, int T, int ks) { return 16 * (2 * wave + t) + pos + (t_s - T) + ks / 3; }

// ---- statistics.  A sigmoid output is >= +0, so its bit pattern orders as an unsigned integer; with the complement of the window
//      index below it, the largest key is the largest score at the smallest window that attains it -- an integer maximum, which does
//      not depend on the order the atomics arrive in.  Key 0 (score +0 at window 2^32 - 1, which no call has) = nothing seen. ----
OWD_HD unsigned long long stat_key(unsigned score_bits, unsigned w) { return ((unsigned long long)score_bits << 32) | (unsigned)~w; }
OWD_HD unsigned stat_key_bits(unsigned long long key) { return (unsigned)(key >> 32); }
OWD_HD unsigned stat_key_window(unsigned long long key) { return ~(unsigned)key; }

// ---- sizes ----
inline uint64_t stats_bytes(int64_t B, int64_t n_ids) { return (uint64_t)B * (uint64_t)n_ids * 12u; }       // int32 count + 64-bit key

// ---- argument checks: nothing has moved when one of them refuses ----
inline int bank_ready_check(const char* fn, bool have_handle, bool committed, int bank_slots) {
    if (!have_handle || !committed) return fail(OWW_ESTATE, "%s: handle not committed", fn);
    if (bank_slots < 1) return fail(OWW_ESTATE, "%s: no bank on this handle (oww_bank_configure before oww_commit)", fn);
    return 0;
}
// live_T[id]: the window length of bank head id, 0 where the slot is empty.  *t_max: the largest T of the listed heads.
inline int bank_ids_check(const char* fn, const int32_t* ids, int64_t n_ids, const int* live_T, int64_t capacity, int* t_max) {
    if (!ids || n_ids < 1) return fail(OWW_EINVAL, "%s: bad argument (n_ids = %lld, need a list of at least one bank id)", fn, (long long)n_ids);
    int tm = 0;
    for (int64_t i = 0; i < n_ids; ++i) {
        if (ids[i] < 0 || ids[i] >= capacity || live_T[ids[i]] < 1) return fail(OWW_EINVAL, "%s: %d is not a bank head (entry %lld of the list)", fn, ids[i], (long long)i);
        tm = std::max(tm, live_T[ids[i]]);
    }
    *t_max = tm;
    return 0;
}
inline int bank_sizes_check(const char* fn, int64_t B, int64_t n_rows, int64_t t_max, int64_t n_ids, bool matrix) {
    const int64_t nw = n_win(n_rows, t_max);
    const uint64_t fb = feats_bytes(B, n_rows), ob = matrix ? out_bytes(B, nw, n_ids) : stats_bytes(B, n_ids);
    // (no product wraps: B, n_rows, n_ids < 2^31, and the matrix's three-way product is compared by division)
    if (fb > kMaxBytes || (matrix && (uint64_t)B * (uint64_t)nw > kMaxBytes / ((uint64_t)n_ids * 4u)) || ob > kMaxBytes ||
        (uint64_t)B * (uint64_t)n_rows > (uint64_t)INT64_MAX / 1024)
        return fail(OWW_ENOMEM, "%s: %llu bytes of features and %llu bytes of %s do not fit", fn, (unsigned long long)fb, (unsigned long long)ob,
                    matrix ? "scores" : "statistics");
    if (B * tiles_per_seq(nw, kWavesSmall) > kMaxGrid)
        return fail(OWW_ENOMEM, "%s: %lld sequences x %lld tiles exceed one launch (%llu bytes of features); score in chunks", fn, (long long)B,
                    (long long)tiles_per_seq(nw, kWavesSmall), (unsigned long long)fb);
    return 0;
}
inline int bank_features_check(const char* fn, const void* feats, int feats_on_device, int64_t B, int64_t n_rows, int64_t t_max, int64_t n_ids,
                               const void* out, int out_on_device) {
    if (!feats || !out || B < 1) return fail(OWW_EINVAL, "%s: bad argument (B = %lld, null features or output)", fn, (long long)B);
    if (int rc = rows_check(fn, feats, feats_on_device, n_rows, t_max)) return rc;
    if (out_on_device && (reinterpret_cast<uintptr_t>(out) & 15)) return fail(OWW_EINVAL, "%s: a device output must be 16-byte aligned", fn);
    return bank_sizes_check(fn, B, n_rows, t_max, n_ids, true);
}
inline int bank_stats_check(const char* fn, const void* feats, int feats_on_device, int64_t B, int64_t n_rows, int64_t t_max, int64_t n_ids,
                            const float* thresholds, const void* count, const void* max, const void* argmax) {
    if (!feats || !count || !max || !argmax || B < 1) return fail(OWW_EINVAL, "%s: bad argument (B = %lld, null features or output)", fn, (long long)B);
    if (int rc = rows_check(fn, feats, feats_on_device, n_rows, t_max)) return rc;
    if (thresholds)
        for (int64_t i = 0; i < n_ids; ++i)
            if (std::isnan(thresholds[i])) return fail(OWW_EINVAL, "%s: threshold %lld is NaN", fn, (long long)i);
    return bank_sizes_check(fn, B, n_rows, t_max, n_ids, false);
}

}  // namespace owd
