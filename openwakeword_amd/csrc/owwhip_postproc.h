// owwhip_postproc.h -- Model.predict's post-processing (the reference's model.py:330-381), once: the score rule (first-five zeroing,
// patience or debounce over the pair's score ring, ring append), the VAD gate over ring[-7:-4], the VAD ring's push and clear, and the
// two parameter blocks every launch site hands to them.  Three kernels run it -- owk::postproc_kernel, the epilogue of
// owh::heads_hx_kernel and owh::bank_post_kernel -- and a handle moves between the first two whenever its call length changes, so the
// three must be one piece of code.  Free of HIP, like owwhip_dense_host.h: the kernels include it for the device, and
// tests/postproc_check.cpp includes it alone and runs the same functions on the host under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "owwhip.h"

#ifdef __HIPCC__
#define OWQ_HD __host__ __device__ __forceinline__
#else
#define OWQ_HD inline
#endif

namespace owq {

constexpr int kScoreRing = 30;        // prediction_buffer maxlen (model.py:198): final ungated scores per (stream, label) or (stream, slot)
static_assert(kScoreRing == OWW_SCORE_RING, "the score ring's depth is part of the ABI");
constexpr uint32_t kWarmup = 5;       // predictions zeroed while the ring holds fewer (model.py:331-333)
constexpr int kVadRing = 8;           // VAD scores kept per stream: a power of two that covers the gate's window
// the gate's window, vad ring[-7:-4] (model.py:375-381): entries L - kGateOldest .. L - kGateNewest of the L pushed so far, none while
// L < kGateNewest
constexpr uint32_t kGateOldest = 7, kGateNewest = 5;
static_assert((kVadRing & (kVadRing - 1)) == 0 && (uint32_t)kVadRing > kGateOldest, "slot = L & (kVadRing - 1) must keep the window");

struct Rules {
    const int* patience;     // [labels] or [bank heads]; > 0 selects the patience rule
    const float* threshold;  // same index (NaN = no threshold: never debounced)
    int debounce_frames;     // handle-wide
};
struct Gate {
    const float* vad_ring;   // [S][kVadRing]
    const uint32_t* n_vad;   // [S] scores pushed so far
    float vad_threshold;     // <= 0: gate off
};

// One (stream, label) or (stream, slot) pair of one predict(): `raw` is the pair's score of this call, `cnt` the predictions its ring has
// taken so far, r.patience[idx] / r.threshold[idx] its rule (read only where a rule can apply).  Appends the final UNGATED score to the
// ring and returns it.
OWQ_HD float score_rule(float raw, uint32_t cnt, float* ring, const Rules& r, int idx) {
    const int have = cnt < (uint32_t)kScoreRing ? (int)cnt : kScoreRing;
    float sc = raw;
    if (cnt < kWarmup) sc = 0.0f;                                           // model.py:331-333
    if (sc != 0.0f) {
        const int pat = r.patience[idx];
        const float thr = r.threshold[idx];
        if (pat > 0) {                                                      // model.py:349-352
            const int look = pat < have ? pat : have;
            int n_ok = 0;
            for (int i = 1; i <= look; ++i) n_ok += ring[(cnt - i) % (uint32_t)kScoreRing] >= thr ? 1 : 0;
            if (n_ok < pat) sc = 0.0f;
        } else if (r.debounce_frames > 0 && thr == thr) {                   // model.py:353-359
            const int look = r.debounce_frames < have ? r.debounce_frames : have;
            int n_hit = 0;
            for (int i = 1; i <= look; ++i) n_hit += ring[(cnt - i) % (uint32_t)kScoreRing] >= thr ? 1 : 0;
            if (sc >= thr && n_hit > 0) sc = 0.0f;
        }
    }
    ring[cnt % (uint32_t)kScoreRing] = sc;                                  // model.py:362-363
    return sc;
}

// model.py:375-381 on one stream's VAD ring with L scores pushed: closed (the step's returned scores are zeroed; the score ring keeps the
// ungated values) when the largest score of the window is below the threshold -- 0 while the window is empty.  (L counts the pushes since
// the stream's last VAD reset; the window's arithmetic takes L + kGateNewest not to wrap -- 2^32 pushes are ten years of audio.)
OWQ_HD bool gate_closed(const float* vad_ring, uint32_t L, float vad_threshold) {
    if (!(vad_threshold > 0.0f)) return false;
    float vmax = 0.0f;
    if (L >= kGateNewest) {
        vmax = -INFINITY;
        for (uint32_t i = (L >= kGateOldest ? L - kGateOldest : 0u); i + kGateNewest <= L; ++i) vmax = fmaxf(vmax, vad_ring[i & (uint32_t)(kVadRing - 1)]);
    }
    return vmax < vad_threshold;
}
OWQ_HD bool gate_closed(const Gate& g, size_t s) {                          // (the count is read only where the gate is on)
    return g.vad_threshold > 0.0f && gate_closed(g.vad_ring + s * kVadRing, g.n_vad[s], g.vad_threshold);
}

OWQ_HD void vad_push(float* vad_ring, uint32_t* n_vad, size_t s, float v) {
    const uint32_t L = n_vad[s];
    vad_ring[s * kVadRing + (L & (uint32_t)(kVadRing - 1))] = v;
    n_vad[s] = L + 1u;
}
OWQ_HD void vad_clear(float* vad_ring, uint32_t* n_vad, size_t s) {
    for (int i = 0; i < kVadRing; ++i) vad_ring[s * kVadRing + i] = 0.f;
    n_vad[s] = 0u;
}

}  // namespace owq
