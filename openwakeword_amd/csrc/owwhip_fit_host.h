// owwhip_fit_host.h -- what the host computes for the device-side custom-verifier fit (include/owwhip.h: oww_verifier_fit; the
// reference: custom_verifier_model.py:95-113): the argument checks and 64-bit sizes, the walk over the offsets (class counts, N and
// the per-problem refusals known before any launch), the slab plan under a scratch budget, the triangular tile grid of the batched
// Gram kernel, and the solver's constants.  Host only and free of HIP: owwhip.hip includes it for the library, owwhip_fit.h for the
// records the kernels read, tests/fit_check.cpp includes it alone under AddressSanitizer / UBSan, where tests/verifier_fit_ref.py
// restates the plan and the map.
#pragma once
#include <cstdint>
#include "owwhip_pack.h"

namespace owf {

using owp::fail;

constexpr int kTile = 32;                  // rows and columns of one wave's Gram tile (2 x 2 MFMA tiles of 16)
constexpr int kMaxN = OWW_FIT_MAX_N;
constexpr int kNewtonCap = 40;             // Newton steps; a problem that reaches it unconverged is OWW_FIT_NOT_CONVERGED
// The stop rule: res = max_i |a_i + C (p_i - y_i)| / C <= kEpsStop.  Residual floors of the fp32 restatement (tests/verifier_fit_ref.py:
// fit32 run to the cap, smallest res of the run) over the test's case table: N = 2: 0; N = 15 .. 200 at T = 16 / 34, C = 0.001 / 0.1,
// every regime: 1.9e-8 .. 9.2e-8; N = 1024: 1.16e-7; N = 200 at T = 1 (more windows than features), C = 0.1: 1.86e-7.
// kEpsStop = 8 x the largest.
constexpr float kEpsStop = 1.5e-6f;
constexpr float kCgRtol2 = 1e-10f;         // the inner conjugate gradients stop at |r|^2 <= kCgRtol2 |rhs|^2 ...
constexpr int cg_cap(int N) { return 2 * N + 32; }    // ... or after this many steps
constexpr float kJNoise = 1e-5f;           // a step is halved only where J rises by more than kJNoise |J| (fp32 noise of J)
constexpr int kMaxHalvings = 8;
constexpr long long kDefaultBudget = 1ll << 30;    // scratch bytes of one slab (OWW_FIT_SCRATCH_BYTES overrides, read at the call)

// one problem of a slab, as the kernels read it
struct Problem {
    long long x_off;         // floats from the slab's window base to the problem's first window
    long long z_row;         // its first row in the slab's Z halves
    long long k_off;         // floats from the slab's Gram base to its [N][N] matrix
    long long y_off;         // its first label in the slab's labels
    int32_t N, id, u, pad;   // windows, pool slot, index in the call
};
static_assert(sizeof(Problem) == 48, "Problem is three 16-byte loads");

// the record a problem's workgroup leaves (solver) -- what comes back to the host
struct Record { int32_t status, iterations; float residual, pad; };

struct Tile { int32_t p, tr, tc, pad; };   // problem of the slab, tile row, tile column (tc >= tr)

inline long long tile_count(int N) { const long long nt = (N + kTile - 1) / kTile; return nt * (nt + 1) / 2; }

// scratch bytes of one problem: staged windows (host windows only), Z hi + lo, Gram matrix, mu / s (fp64 each), a / flags
inline long long problem_bytes(int N, long long D, bool on_device) {
    return (on_device ? 0 : (long long)N * D * 4) + 2ll * N * D * 2 + (long long)N * N * 4 + D * 16 + (long long)N * 8;
}

// ---- whole-call checks: nothing has moved when one refuses ----
inline int check_args(bool committed, int pool_cap, const void* windows, const int64_t* offsets, const uint8_t* labels, int32_t U, int32_t T, int TR, float C,
                      const void* out) {
    if (!committed || pool_cap == 0) return fail(OWW_ESTATE, "oww_verifier_fit: needs oww_verifier_configure before oww_commit, and a committed handle");
    if (U < 0 || !offsets || (U > 0 && !out)) return fail(OWW_EINVAL, "oww_verifier_fit: bad argument");
    if (T < 1 || T > TR) return fail(OWW_EINVAL, "oww_verifier_fit: T = %d outside 1 .. %d (the handle's feature ring)", T, TR);
    if (!std::isfinite(C) || !(C > 0.f)) return fail(OWW_EINVAL, "oww_verifier_fit: C = %g (finite and > 0)", (double)C);
    if (offsets[0] < 0) return fail(OWW_EINVAL, "oww_verifier_fit: offsets[0] = %lld", (long long)offsets[0]);
    for (int u = 0; u < U; ++u)
        if (offsets[u + 1] < offsets[u]) return fail(OWW_EINVAL, "oww_verifier_fit: offsets not ascending at problem %d", u);
    // windows x floats of the whole call as a 64-bit byte count that still fits
    const long long D = (long long)T * OWW_EMB_DIM;
    if (offsets[U] > (long long)(INT64_MAX / 4) / D) return fail(OWW_EINVAL, "oww_verifier_fit: %lld windows of %lld floats overflow 64-bit sizes", (long long)offsets[U], D);
    if (offsets[U] > offsets[0] && (!windows || !labels)) return fail(OWW_EINVAL, "oww_verifier_fit: null windows or labels");
    for (long long i = offsets[0]; i < offsets[U]; ++i)
        if (labels[i] > 1) return fail(OWW_EINVAL, "oww_verifier_fit: label %d at window %lld (0 or 1)", (int)labels[i], i);
    return 0;
}

// ---- the offsets walk: per-problem status known on the host (BAD_N, ONE_CLASS; OK = goes to the device), class counts ----
inline void classify(const int64_t* offsets, const uint8_t* labels, int32_t U, oww_fit_result* out) {
    for (int u = 0; u < U; ++u) {
        const long long n = offsets[u + 1] - offsets[u];
        oww_fit_result r{};
        r.id = -1;
        r.residual = 0.f;
        if (n < 2 || n > kMaxN) r.status = OWW_FIT_BAD_N;
        else {
            for (long long i = offsets[u]; i < offsets[u + 1]; ++i) r.n_pos += labels[i];
            r.n_neg = (int32_t)n - r.n_pos;
            r.status = (r.n_pos == 0 || r.n_neg == 0) ? OWW_FIT_ONE_CLASS : OWW_FIT_OK;
        }
        out[u] = r;
    }
}

// gives every problem that passed classify() a free pool slot (lowest first, as oww_verifier_add); refuses the call when they do not fit
inline int assign_ids(const std::vector<int>& pool_T, int32_t U, oww_fit_result* out) {
    long long need = 0, free_n = 0;
    for (int u = 0; u < U; ++u) need += out[u].status == OWW_FIT_OK;
    for (int t : pool_T) free_n += t == 0;
    if (need > free_n) return fail(OWW_EINVAL, "oww_verifier_fit: %lld problems to fit, %lld free pool slots (capacity %d)", need, free_n, (int)pool_T.size());
    size_t v = 0;
    for (int u = 0; u < U; ++u) {
        if (out[u].status != OWW_FIT_OK) continue;
        while (pool_T[v] != 0) ++v;
        out[u].id = (int32_t)v++;
    }
    return 0;
}

// ---- the slab plan: consecutive whole problems (of those that run), greedily while the slab's bytes stay within the budget; a
//      problem larger than the budget is a slab of its own ----
struct Slab { int first, last; long long rows, k_floats, tiles; };     // problems [first, last) of the run list
inline std::vector<Slab> slab_plan(const std::vector<int>& Ns, long long D, long long budget, bool on_device) {
    std::vector<Slab> slabs;
    Slab cur{0, 0, 0, 0, 0};
    long long used = 0;
    for (int i = 0; i < (int)Ns.size(); ++i) {
        const long long need = problem_bytes(Ns[i], D, on_device);
        if (cur.last > cur.first && used + need > budget) { slabs.push_back(cur); cur = Slab{i, i, 0, 0, 0}; used = 0; }
        cur.last = i + 1;
        cur.rows += Ns[i];
        cur.k_floats += (long long)Ns[i] * Ns[i];
        cur.tiles += tile_count(Ns[i]);
        used += need;
    }
    if (cur.last > cur.first) slabs.push_back(cur);
    return slabs;
}

// the triangular Gram grid of a slab: problem-major, tile-row-major, tiles on or above the diagonal
inline std::vector<Tile> tile_map(const std::vector<int>& Ns, int first, int last) {
    std::vector<Tile> tiles;
    for (int i = first; i < last; ++i) {
        const int nt = (Ns[i] + kTile - 1) / kTile;
        for (int r = 0; r < nt; ++r) for (int c = r; c < nt; ++c) tiles.push_back(Tile{i - first, r, c, 0});
    }
    return tiles;
}

}  // namespace owf
