// owwhip_autotrain_host.h -- what the host computes for validating, checkpointing and merging the heads of a training session
// (include/owwhip.h: oww_train_new_sequence .. oww_train_get_slot; the reference: Model.auto_train, train.py:261-366, its validation
// pass train.py:512-553 and average_models train.py:198-223): the argument checks, the 64-bit sizes of the eval tables and of the
// checkpoint slots, the tile plan of train_eval_kernel.  Host only and free of HIP: owwhip.hip includes it for the library,
// owwhip_autotrain.h for the records the kernels read, tests/auto_train_check.cpp includes it alone under AddressSanitizer / UBSan,
// where tests/auto_train_ref.py restates sizes, plan and refusals.
#pragma once
#include <cstdint>
#include "owwhip_train_host.h"

namespace owa {

using owp::fail;

constexpr int kEvalMaxRows = OWW_TRAIN_EVAL_MAX_ROWS;      // slots of one oww_train_eval call
constexpr int kMaxSlots = 65535;                           // checkpoint slots per problem
constexpr int kCounts = 5;                                 // n_pos, n_neg, pos_gt, neg_gt, neg_ge
static_assert(sizeof(oww_train_counts) == kCounts * sizeof(int32_t), "oww_train_counts is five int32");

// ---- the tile plan and the sizes of one eval call ----
struct EvalPlan {
    int n_tiles;                           // tiles of owt::kTileRows slots: the grid is (problems, n_tiles), problems fastest
    long long table, scores;               // entries of idx / y [rows][n]; floats of the score buffer [U][n] (0 without scores)
};
inline EvalPlan eval_plan(int U, int n, int shared, bool scores) {
    EvalPlan p{};
    p.n_tiles = (n + owt::kTileRows - 1) / owt::kTileRows;
    p.table = (long long)(shared ? 1 : U) * n;
    p.scores = scores ? (long long)U * n : 0;
    return p;
}

// floats of the checkpoint slots [C][U][stride]; false when the byte count overflows 64 bits
inline bool slot_floats(int32_t C, int32_t U, long long stride, long long* out) {
    if (C < 1 || U < 1 || stride < 1) return false;
    const long long per = (long long)U * stride;           // U <= 65535, stride < 2^31: fits
    if (per > (INT64_MAX / 4) / C) return false;
    *out = per * C;
    return true;
}

// ---- checks: nothing has moved when one refuses ----
inline int check_new_sequence(bool open) {
    if (!open) return fail(OWW_ESTATE, "oww_train_new_sequence: no training session on this handle");
    return 0;
}

inline int check_eval_pool(bool open, const float* pool, int64_t P, int T) {
    if (!open) return fail(OWW_ESTATE, "oww_train_set_eval_pool: no training session on this handle");
    if (!pool || P < 1) return fail(OWW_EINVAL, "oww_train_set_eval_pool: %lld windows", (long long)P);
    if (P > INT32_MAX) return fail(OWW_EINVAL, "oww_train_set_eval_pool: %lld windows (an index is 32 bits)", (long long)P);
    if (P > (INT64_MAX / 4) / ((long long)T * OWW_EMB_DIM)) return fail(OWW_EINVAL, "oww_train_set_eval_pool: %lld windows overflow 64-bit sizes", (long long)P);
    return 0;
}

// what can be refused before the tables are read (the sizes of the tables rest on these)
inline int check_eval_head(bool open, int64_t EP, int32_t C, int32_t source, int32_t n, const int32_t* idx, const uint8_t* y, const void* counts) {
    if (!open) return fail(OWW_ESTATE, "oww_train_eval: no training session on this handle");
    if (EP < 1) return fail(OWW_ESTATE, "oww_train_eval: no eval pool (oww_train_set_eval_pool first)");
    if (source < -1) return fail(OWW_EINVAL, "oww_train_eval: source %d (-1 = the live parameters, or a checkpoint slot)", source);
    if (source >= 0 && C < 1) return fail(OWW_ESTATE, "oww_train_eval: source %d, but no checkpoint slots (oww_train_checkpoints first)", source);
    if (source >= C && source >= 0) return fail(OWW_EINVAL, "oww_train_eval: source %d of %d checkpoint slots", source, C);
    if (n < 1 || n > kEvalMaxRows) return fail(OWW_EINVAL, "oww_train_eval: n = %d slots (1 .. %d)", n, kEvalMaxRows);
    if (!idx || !y || !counts) return fail(OWW_EINVAL, "oww_train_eval: null argument");
    return 0;
}

// idx / y: host copies of the tables, [rows][n] with rows = 1 (shared) or U
inline int check_eval(bool open, int64_t EP, int32_t C, int32_t U, int32_t source, int32_t n, const int32_t* idx, const uint8_t* y, int shared,
                      const void* counts) {
    if (int rc = check_eval_head(open, EP, C, source, n, idx, y, counts)) return rc;
    const long long total = (long long)(shared ? 1 : U) * n;
    for (long long i = 0; i < total; ++i) {
        if (idx[i] < -1 || idx[i] >= EP) return fail(OWW_EINVAL, "oww_train_eval: index %d at entry %lld (-1 .. %lld)", idx[i], i, (long long)EP - 1);
        if (y[i] > 1) return fail(OWW_EINVAL, "oww_train_eval: label %d at entry %lld (0 or 1)", (int)y[i], i);
    }
    return 0;
}

inline int check_checkpoints(bool open, int32_t C, int32_t U, long long stride, long long* floats) {
    if (!open) return fail(OWW_ESTATE, "oww_train_checkpoints: no training session on this handle");
    if (C < 1 || C > kMaxSlots) return fail(OWW_EINVAL, "oww_train_checkpoints: %d slots (1 .. %d)", C, kMaxSlots);
    if (!slot_floats(C, U, stride, floats)) return fail(OWW_EINVAL, "oww_train_checkpoints: %d slots x %d problems overflow 64-bit sizes", C, U);
    return 0;
}

inline int check_snapshot(bool open, int32_t C, int32_t U, const int32_t* slot) {
    if (!open) return fail(OWW_ESTATE, "oww_train_snapshot: no training session on this handle");
    if (C < 1) return fail(OWW_ESTATE, "oww_train_snapshot: no checkpoint slots (oww_train_checkpoints first)");
    if (!slot) return fail(OWW_EINVAL, "oww_train_snapshot: null argument");
    for (int u = 0; u < U; ++u)
        if (slot[u] < -1 || slot[u] >= C) return fail(OWW_EINVAL, "oww_train_snapshot: slot %d for problem %d (-1 .. %d)", slot[u], u, C - 1);
    return 0;
}

inline int check_average(bool open, int32_t C, const uint8_t* sel, int32_t dst) {
    if (!open) return fail(OWW_ESTATE, "oww_train_average: no training session on this handle");
    if (C < 1) return fail(OWW_ESTATE, "oww_train_average: no checkpoint slots (oww_train_checkpoints first)");
    if (!sel) return fail(OWW_EINVAL, "oww_train_average: null argument");
    if (dst < 0 || dst >= C) return fail(OWW_EINVAL, "oww_train_average: destination slot %d of %d", dst, C);
    return 0;
}

inline int check_get_slot(bool open, int32_t C, int32_t U, int32_t u, int32_t slot, const float* params, int64_t n_params, long long n) {
    if (!open) return fail(OWW_ESTATE, "oww_train_get_slot: no training session on this handle");
    if (C < 1) return fail(OWW_ESTATE, "oww_train_get_slot: no checkpoint slots (oww_train_checkpoints first)");
    if (u < 0 || u >= U) return fail(OWW_EINVAL, "oww_train_get_slot: problem %d of %d", u, U);
    if (slot < 0 || slot >= C) return fail(OWW_EINVAL, "oww_train_get_slot: slot %d of %d", slot, C);
    if (!params || n_params != n) return fail(OWW_EINVAL, "oww_train_get_slot: room for %lld floats, a record has %lld", (long long)n_params, n);
    return 0;
}

}  // namespace owa
