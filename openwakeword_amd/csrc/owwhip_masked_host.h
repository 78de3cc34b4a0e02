// owwhip_masked_host.h -- what the host computes for a masked step with few participants (include/owwhip.h: oww_step_masked,
// oww_submit_masked): the participation rule and the five group lists -- stream ids, then the groups of 2 / 4 / 8 / 16 streams that hold
// a participant -- that the launches of stages B..E, the heads and the VAD LSTM index the device through (StepArgs::gl).  Host only and
// free of HIP: owwhip.hip includes it for the library (build_active_lists: staging, upload, StepArgs), tests/planners_check.cpp includes
// it alone under AddressSanitizer / UBSan.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

namespace owl {

// ---- participation: the number of streams that take part; 0 = nothing to do, -1 = use the dense launches (more than 7/8 of the
//      streams take part: the lists then save nothing; below that they do even for a mask that touches most groups, and a serving edge
//      that places connections by cohort -- serve.py::SlotAllocator -- makes participation per group all-or-nothing, so the launches
//      shrink with the mask) ----
inline int participants(const uint8_t* on, int S) {
    int n_act = 0;
    for (int s = 0; s < S; ++s) n_act += on[s] != 0;          // (vectorised by the compiler)
    return (long long)n_act * 8 > (long long)S * 7 ? -1 : n_act;
}

// ---- the lists.  List k is the ascending list of distinct s / G_k over the participating streams, G = 1, 2, 4, 8, 16; packed back to
//      back in that order: list k is out[off[k] .. off[k] + n[k]).  One pass over the mask, eight streams (one 64-bit word = one stage-E
//      group) at a time; the five lists grow side by side in fixed regions of `out` (lists_capacity(S) ints) and are packed afterwards.
//      Returns the number of participants (= n[0]); a mask that is all off writes nothing. ----
inline size_t lists_capacity(int S) { return (size_t)S + S / 2 + S / 4 + S / 8 + S / 16 + 64; }
inline int build_lists(const uint8_t* on, int S, int* out, int n[5], size_t off[5]) {
    const size_t base[5] = {0, (size_t)S, (size_t)S + S / 2 + 8, (size_t)S + S / 2 + S / 4 + 16, (size_t)S + S / 2 + S / 4 + S / 8 + 24};
    for (int k = 0; k < 5; ++k) n[k] = 0;
    const int W8 = S / 8;
    int last_v = -1;
    auto visit = [&](int s0, const uint8_t* b, int cnt) {        // streams s0 .. s0+cnt-1 (cnt <= 8), at least one of them on
        const int g8 = s0 / 8;
        out[base[3] + n[3]++] = g8;
        if (g8 / 2 != last_v) { last_v = g8 / 2; out[base[4] + n[4]++] = g8 / 2; }
        for (int q = 0; q < cnt; q += 4) {
            bool any4 = false;
            for (int c = q; c < std::min(cnt, q + 4); c += 2) {
                bool any2 = false;
                for (int i = c; i < std::min(cnt, c + 2); ++i) if (b[i]) { out[base[0] + n[0]++] = s0 + i; any2 = true; }
                if (any2) { out[base[1] + n[1]++] = (s0 + c) / 2; any4 = true; }
            }
            if (any4) out[base[2] + n[2]++] = (s0 + q) / 4;
        }
    };
    for (int w = 0; w < W8; ++w) {
        uint64_t v;
        memcpy(&v, on + (size_t)w * 8, 8);
        if (v) visit(w * 8, on + (size_t)w * 8, 8);
    }
    if (S % 8) {
        bool any = false;
        for (int s = W8 * 8; s < S; ++s) any = any || on[s] != 0;
        if (any) visit(W8 * 8, on + (size_t)W8 * 8, S - W8 * 8);
    }
    size_t at = 0;
    for (int k = 0; k < 5; ++k) {
        if (base[k] != at) memmove(out + at, out + base[k], (size_t)n[k] * sizeof(int));
        off[k] = at;
        at += (size_t)n[k];
    }
    return n[0];
}

}  // namespace owl
