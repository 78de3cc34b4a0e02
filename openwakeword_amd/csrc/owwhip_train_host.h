// owwhip_train_host.h -- what the host computes for training bank heads on the device (include/owwhip.h: oww_train_*; the reference:
// train.py:434-510, one step of Model.train_model for the network of train.py:66-83 with n_blocks = 1, n_classes = 1): the argument
// checks and 64-bit sizes, the flat parameter record's layout, the tile plan of the three kernels and their scratch sizes.  Host only
// and free of HIP: owwhip.hip includes it for the library, owwhip_train.h for the records the kernels read, tests/train_check.cpp
// includes it alone under AddressSanitizer / UBSan, where tests/head_train_ref.py restates layout, plan and refusals.
#pragma once
#include <cstdint>
#include "owwhip_pack.h"

namespace owt {

using owp::fail;

constexpr int kTileRows = 64;              // batch rows of one forward / backward workgroup (4 waves x 16 MFMA rows)
constexpr int kMaxBatch = OWW_TRAIN_MAX_BATCH;
constexpr int kMaxSteps = OWW_TRAIN_MAX_STEPS;
constexpr int kMaxProblems = 65535;
constexpr int kAccumulate = 128;           // train.py:492: fewer kept samples than this accumulate and skip
constexpr float kSelNeg = 0.001f;          // train.py:464: a negative is kept at p >= this
constexpr float kSelPos = 0.999f;          // train.py:465: a positive is kept at p < this

// ---- the flat parameter record of one problem (floats): the bank head's own fields, in its order and orientation ----
struct Layout {
    long long F, D;                        // 96 T inputs, hidden units
    long long w1, b1, g1, be1, w2, b2, g2, be2, w3, b3;     // offsets
    long long n;                           // floats of the record (= oww_train_param_count)
    long long stride;                      // floats from one problem's record to the next on the device (n rounded up to 4)
    long long small;                       // floats behind w1: what the third kernel owns
};
inline Layout layout(int T, int D) {
    Layout L{};
    L.F = (long long)T * OWW_EMB_DIM; L.D = D;
    L.w1 = 0;
    L.b1 = L.F * D; L.g1 = L.b1 + D; L.be1 = L.g1 + D;
    L.w2 = L.be1 + D;
    L.b2 = L.w2 + (long long)D * D; L.g2 = L.b2 + D; L.be2 = L.g2 + D;
    L.w3 = L.be2 + D; L.b3 = L.w3 + D;
    L.n = L.b3 + 1;
    L.stride = (L.n + 3) / 4 * 4;
    L.small = L.n - L.b1;
    return L;
}

// the counters a problem carries from step to step (train.py:443-444 and Adam's step count)
struct Counters { int32_t acc_steps, acc_samples, opt_steps, pad; };

// what a step leaves per (problem, step): history["loss"]'s value (NaN where no optimizer step was taken) and the kept count m
struct StepRecord { float loss; int32_t m; };
static_assert(sizeof(StepRecord) == sizeof(oww_train_record), "StepRecord is oww_train_record");

// ---- the tile plan and the scratch of one steps call ----
struct Plan {
    int n_tiles, n_pad;                    // tiles of kTileRows batch rows; rows with the padding
    long long dz1, part, tile_words;       // floats of dZ1 [U][n_pad][D]; of the tile partials [U][n_tiles][small]; tile counts / losses [U][n_tiles]
    int w1_groups;                         // workgroups of the W1 kernel per problem: 64 input columns each (4 waves x 16)
};
inline Plan plan(int U, int T, int D, int n_batch) {
    const Layout L = layout(T, D);
    Plan p{};
    p.n_tiles = (n_batch + kTileRows - 1) / kTileRows;
    p.n_pad = p.n_tiles * kTileRows;
    p.dz1 = (long long)U * p.n_pad * D;
    p.part = (long long)U * p.n_tiles * L.small;
    p.tile_words = (long long)U * p.n_tiles;
    p.w1_groups = (int)((L.F + 63) / 64);
    return p;
}

// ---- checks: nothing has moved when one refuses ----
inline int check_begin(bool committed, bool open, int32_t U, int32_t T, int32_t D, int TR, const float* params) {
    if (!committed) return fail(OWW_ESTATE, "oww_train_begin: needs a committed handle");
    if (open) return fail(OWW_ESTATE, "oww_train_begin: a training session is open on this handle (oww_train_end first)");
    if (U < 1 || U > kMaxProblems) return fail(OWW_EINVAL, "oww_train_begin: %d problems (1 .. %d)", U, kMaxProblems);
    if (D < 16 || D > 128 || D % 16) return fail(OWW_EINVAL, "oww_train_begin: hidden = %d (a multiple of 16 in 16 .. 128)", D);
    if (T < 1 || T > TR) return fail(OWW_EINVAL, "oww_train_begin: T = %d outside 1 .. %d (the handle's feature ring)", T, TR);
    if (!params) return fail(OWW_EINVAL, "oww_train_begin: null parameters");
    return 0;
}

inline int check_pool(bool open, const float* pool, int64_t P, int T) {
    if (!open) return fail(OWW_ESTATE, "oww_train_set_pool: no training session on this handle");
    if (!pool || P < 1) return fail(OWW_EINVAL, "oww_train_set_pool: %lld windows", (long long)P);
    if (P > INT32_MAX) return fail(OWW_EINVAL, "oww_train_set_pool: %lld windows (an index is 32 bits)", (long long)P);
    if (P > (INT64_MAX / 4) / ((long long)T * OWW_EMB_DIM)) return fail(OWW_EINVAL, "oww_train_set_pool: %lld windows overflow 64-bit sizes", (long long)P);
    return 0;
}

// idx / y: host copies of the tables, [rows][K][n_batch] with rows = 1 (shared) or U
inline int check_steps(bool open, int64_t P, int32_t U, int32_t K, int32_t n_batch, const int32_t* idx, const uint8_t* y, int shared,
                       const double* lr, const float* neg_weight, const void* out) {
    if (!open) return fail(OWW_ESTATE, "oww_train_steps: no training session on this handle");
    if (P < 1) return fail(OWW_ESTATE, "oww_train_steps: no window pool (oww_train_set_pool first)");
    if (K < 1 || K > kMaxSteps) return fail(OWW_EINVAL, "oww_train_steps: K = %d steps (1 .. %d)", K, kMaxSteps);
    if (n_batch < 1 || n_batch > kMaxBatch) return fail(OWW_EINVAL, "oww_train_steps: n_batch = %d (1 .. %d)", n_batch, kMaxBatch);
    if (!idx || !y || !lr || !neg_weight || !out) return fail(OWW_EINVAL, "oww_train_steps: null argument");
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(lr[k]) || lr[k] < 0.0) return fail(OWW_EINVAL, "oww_train_steps: lr[%d] = %g (finite and >= 0)", k, (double)lr[k]);
        if (!std::isfinite(neg_weight[k]) || neg_weight[k] < 0.f)
            return fail(OWW_EINVAL, "oww_train_steps: neg_weight[%d] = %g (finite and >= 0)", k, (double)neg_weight[k]);
    }
    const long long rows = shared ? 1 : U, total = rows * K * n_batch;
    for (long long i = 0; i < total; ++i) {
        if (idx[i] < -1 || idx[i] >= P) return fail(OWW_EINVAL, "oww_train_steps: index %d at entry %lld (-1 .. %lld)", idx[i], i, (long long)P - 1);
        if (y[i] > 1) return fail(OWW_EINVAL, "oww_train_steps: label %d at entry %lld (0 or 1)", (int)y[i], i);
    }
    return 0;
}

}  // namespace owt
