// owwhip_verifier_host.h -- what the host computes for the per-stream custom verifiers (include/owwhip.h: oww_assign_verifiers,
// oww_bank_assign_verifiers, oww_verifier_*): the entry of stream_verifier_kernel's list (owwhip_kernels.h), the list itself from the
// assignment tables, and the argument checks and bookkeeping of an assignment.  Host only and free of HIP: owwhip.hip includes it for
// the library (sv_rebuild: upload, counter reset), owwhip_kernels.h for the entry, tests/planners_check.cpp includes it alone under
// AddressSanitizer / UBSan, where tests/verifier_budget.py::sv_list is held to it.
#pragma once
#include "owwhip_pack.h"

namespace owk {
struct SvEntry {
    int32_t s;               // stream
    int16_t col;             // >= 0: fixed score column; < 0: bank slot ~col
    int16_t T;               // feature rows of the verifier (= of the column's model / the slot's head)
    int32_t v;               // >= 0: pool verifier; < 0: the handle-wide verifier of column ~v
    float thr;               // re-score when raw >= thr (model.py:322)
};
static_assert(sizeof(SvEntry) == 16, "SvEntry is one 16-byte load");
constexpr int SV_PAIRS = 16;     // entries per wave
}  // namespace owk

namespace owsv {

using owk::SvEntry;
using owp::fail;

// pairs whose assignment is not the default: > 0 switches from verifier_kernel to stream_verifier_kernel
inline long long count_assigned(const std::vector<int>& fix, const std::vector<int>& bank) {
    long long n = 0;
    for (const auto* tab : {&fix, &bank}) for (int v : *tab) n += v != OWW_VERIFIER_DEFAULT;
    return n;
}

// The list stream_verifier_kernel walks, from the assignment tables (fix [S][NL], bank [S][K]: pool id, OWW_VERIFIER_DEFAULT or
// OWW_VERIFIER_NONE; their thresholds beside them): stream-major; per stream its fixed columns (a pool verifier, or the column's
// handle-wide verifier -- ver_T [NL] or empty, ver_thr -- where the pair keeps the default), then its bank slots (pool verifiers only).
// Empty while no pair carries a per-stream assignment (n_assigned = 0): verifier_kernel then serves the handle-wide verifiers.
using Ints = std::vector<int>;
using Floats = std::vector<float>;
inline std::vector<SvEntry> sv_list(int S, int NL, int K, const Ints& fix, const Floats& fix_thr, const Ints& bank, const Floats& bank_thr, const Ints& vpool_T,
                                    const Ints& ver_T, const Floats& ver_thr, long long n_assigned) {
    std::vector<SvEntry> list;
    if (n_assigned <= 0) return list;
    list.reserve((size_t)S * NL);
    for (int s = 0; s < S; ++s) {
        for (int c = 0; c < NL; ++c) {
            const size_t at = (size_t)s * NL + c;
            const int v = fix[at];
            if (v >= 0) list.push_back(SvEntry{s, (int16_t)c, (int16_t)vpool_T[v], v, fix_thr[at]});
            else if (v == OWW_VERIFIER_DEFAULT && !ver_T.empty() && ver_T[c] > 0) list.push_back(SvEntry{s, (int16_t)c, (int16_t)ver_T[c], ~c, ver_thr[c]});
        }
        for (int k = 0; k < K; ++k) {
            const size_t at = (size_t)s * K + k;
            const int v = bank[at];
            if (v >= 0) list.push_back(SvEntry{s, (int16_t)~k, (int16_t)vpool_T[v], v, bank_thr[at]});
        }
    }
    return list;
}

// ---- one assignment call: n (stream, verifier, threshold) triples for column / slot `col` of ncol.  model_T(s) = feature rows of the
//      model behind (s, col), < 0 where a bank slot is empty.  Nothing has moved when the check refuses. ----
template <class ModelT>
int assign_check(const char* fn, bool bank, int col, int ncol, const int32_t* stream_ids, int n, const int32_t* verifier_ids, const float* thresholds,
                 int S, const std::vector<int>& vpool_T, ModelT model_T) {
    const int cap = (int)vpool_T.size();
    if (col < 0 || col >= ncol) return fail(OWW_EINVAL, "%s: %s %d outside [0,%d)", fn, bank ? "slot" : "label", col, ncol);
    if (n < 0 || (n > 0 && (!stream_ids || !verifier_ids || !thresholds))) return fail(OWW_EINVAL, "%s: bad argument", fn);
    for (int i = 0; i < n; ++i) {
        const int s = stream_ids[i], v = verifier_ids[i];
        if (s < 0 || s >= S) return fail(OWW_EINVAL, "%s: stream id %d out of range (0..%d)", fn, s, S - 1);
        if (v < OWW_VERIFIER_NONE || v >= cap || (v >= 0 && vpool_T[v] == 0))
            return fail(OWW_EINVAL, "%s: %d is not a pool verifier, OWW_VERIFIER_DEFAULT or OWW_VERIFIER_NONE (stream %d)", fn, v, s);
        if (v < 0) continue;
        const int T = model_T(s);
        if (T < 0) return fail(OWW_EINVAL, "%s: slot %d of stream %d is empty", fn, col, s);
        if (vpool_T[v] != T)
            return fail(OWW_EINVAL, "%s: verifier %d has T = %d feature rows, the model of stream %d's %s %d has T = %d", fn, v, vpool_T[v], s,
                        bank ? "slot" : "label", col, T);
    }
    return 0;
}
// enters the checked triples into one table [S][ncol] and keeps the count of non-default pairs
inline void assign_apply(std::vector<int>& tab, std::vector<float>& thr, long long& n_assigned, int col, int ncol, const int32_t* stream_ids, int n,
                         const int32_t* verifier_ids, const float* thresholds) {
    for (int i = 0; i < n; ++i) {
        const size_t at = (size_t)stream_ids[i] * ncol + col;
        n_assigned += (verifier_ids[i] != OWW_VERIFIER_DEFAULT) - (tab[at] != OWW_VERIFIER_DEFAULT);
        tab[at] = verifier_ids[i];
        thr[at] = thresholds[i];
    }
}

}  // namespace owsv
