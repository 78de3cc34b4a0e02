// postproc_check.cpp -- the post-processing rule, the VAD gate and the VAD ring push of the library as a plain host program:
// openwakeword_amd/csrc/owwhip_postproc.h alone, no HIP -- the functions the three post-processing kernels call -- built with
// -fsanitize=address,undefined by tests/test_postproc_rules_cpu.py.  Every ring a function touches is malloc'ed at exactly its depth.
//   postproc_check                  the self-checks: prediction counts at the uint32 wrap and the VAD clear, worked by hand below
//   postproc_check IN OUT           the header's answers to the independent cases of IN (uint32 words, float32 values as their bits):
//       IN   n_rule n_gate n_push
//            n_rule x [cnt raw patience threshold debounce_frames ring[30]]
//            n_gate x [L threshold vad_ring[8]]
//            n_push x [L value vad_ring[8]]
//       OUT  n_rule x [score ring[30]]   n_gate x [closed]   n_push x [L vad_ring[8]]
// A failed self-check or a malformed file prints to stderr and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "owwhip_postproc.h"

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "postproc_check: " __VA_ARGS__); fprintf(stderr, " [%s]\n", #cond); ++g_bad; } } while (0)

static float f32(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t u32(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

constexpr int D = owq::kScoreRing, V = owq::kVadRing;

// one pair's rule on buffers of exactly the advertised sizes; the pair's patience and threshold sit at index `idx` of arrays that end there
static float rule_once(float raw, uint32_t cnt, float* ring_io, int pat, float thr, int frames, int idx) {
    float* ring = (float*)malloc(D * sizeof(float));
    int* patience = (int*)malloc((idx + 1) * sizeof(int));
    float* threshold = (float*)malloc((idx + 1) * sizeof(float));
    memcpy(ring, ring_io, D * sizeof(float));
    for (int i = 0; i < idx; ++i) { patience[i] = 31; threshold[i] = 2.0f; }      // (someone else's rule: would refuse everything)
    patience[idx] = pat; threshold[idx] = thr;
    const owq::Rules r{patience, threshold, frames};
    const float sc = owq::score_rule(raw, cnt, ring, r, idx);
    memcpy(ring_io, ring, D * sizeof(float));
    free(ring); free(patience); free(threshold);
    return sc;
}

// ------------------------------------------------------------------------------------------------------------------ self-checks
// 2^32 = 16 (mod 30), so count 0xFFFFFFFF appends to slot 15 and looks back at slots 14, 13, 12, ...; the count after it is 0, where the
// first-five zeroing holds again and no history is read (cnt - i would wrap: the look is min(n, have) = 0 entries).
static void self_checks() {
    const uint32_t top = 0xFFFFFFFFu;
    float ring[D];
    auto fill = [&](float v14, float v13, float v12) {
        for (int i = 0; i < D; ++i) ring[i] = 0.0f;
        ring[15] = 9.0f; ring[14] = v14; ring[13] = v13; ring[12] = v12;
    };
    fill(0.75f, 0.5f, 0.75f);                                   // patience 3 at threshold 0.5: three hits (one by equality) let the score pass
    CHECK(rule_once(0.625f, top, ring, 3, 0.5f, 0, 2) == 0.625f && ring[15] == 0.625f, "patience at the top count: %g, slot 15 %g", ring[15], ring[15]);
    CHECK(ring[14] == 0.75f && ring[13] == 0.5f && ring[12] == 0.75f && ring[16] == 0.0f && ring[0] == 0.0f, "patience at the top count wrote beside slot 15");
    fill(0.75f, 0.75f, 0.25f);                                  // the third entry back misses: refused
    CHECK(rule_once(0.625f, top, ring, 3, 0.5f, 0, 0) == 0.0f && ring[15] == 0.0f, "patience at the top count with a miss at slot 12: slot 15 %g", ring[15]);
    fill(0.75f, 0.75f, 0.25f);                                  // patience 2 does not reach slot 12
    CHECK(rule_once(0.625f, top, ring, 2, 0.5f, 0, 1) == 0.625f && ring[15] == 0.625f, "patience 2 at the top count: slot 15 %g", ring[15]);
    fill(0.25f, 0.5f, 0.25f);                                   // debounce over 2 frames: the hit (by equality) at slot 13 silences a score at the threshold
    CHECK(rule_once(0.5f, top, ring, 0, 0.5f, 2, 0) == 0.0f && ring[15] == 0.0f, "debounce at the top count: slot 15 %g", ring[15]);
    fill(0.25f, 0.5f, 0.25f);                                   // ... over 1 frame it is out of reach
    CHECK(rule_once(0.5f, top, ring, 0, 0.5f, 1, 0) == 0.5f && ring[15] == 0.5f, "debounce of 1 at the top count: slot 15 %g", ring[15]);
    fill(0.25f, 0.5f, 0.25f);                                   // a NaN threshold is no threshold
    CHECK(rule_once(0.5f, top, ring, 0, f32(0x7FC00000u), 30, 3) == 0.5f && ring[15] == 0.5f, "NaN threshold at the top count: slot 15 %g", ring[15]);
    // the count after the top: 0.  A full ring of hits, patience 1 and debounce both armed: the first-five zeroing alone decides
    for (int i = 0; i < D; ++i) ring[i] = 1.0f;
    CHECK(rule_once(0.875f, top + 1u, ring, 1, 0.5f, 30, 0) == 0.0f && ring[0] == 0.0f && ring[1] == 1.0f && ring[D - 1] == 1.0f, "count 0 behind the wrap: slot 0 %g", ring[0]);
    for (int i = 0; i < D; ++i) ring[i] = 1.0f;
    CHECK(rule_once(0.875f, 0u, ring, 0, 0.5f, 30, 0) == 0.0f && ring[0] == 0.0f, "count 0, debounce armed: slot 0 %g", ring[0]);
    // the VAD push at the top count lands in slot 7 and the count wraps to 0; the clear empties one stream's ring and count, not its neighbours'
    float* vr = (float*)malloc(3 * V * sizeof(float));
    uint32_t* nv = (uint32_t*)malloc(3 * sizeof(uint32_t));
    for (int i = 0; i < 3 * V; ++i) vr[i] = 0.25f;
    nv[0] = 3u; nv[1] = top; nv[2] = 11u;
    owq::vad_push(vr, nv, 1, 0.75f);
    CHECK(nv[1] == 0u && vr[V + 7] == 0.75f && vr[V + 6] == 0.25f && vr[2 * V] == 0.25f && nv[0] == 3u && nv[2] == 11u, "push at the top count: count %u, slot 7 %g", nv[1], vr[V + 7]);
    owq::vad_push(vr, nv, 2, 0.5f);                             // 11 & 7 = 3
    CHECK(nv[2] == 12u && vr[2 * V + 3] == 0.5f && vr[2 * V + 2] == 0.25f && vr[2 * V + 4] == 0.25f, "push at count 11: count %u, slot 3 %g", nv[2], vr[2 * V + 3]);
    owq::vad_clear(vr, nv, 1);
    bool clean = nv[1] == 0u && nv[0] == 3u && nv[2] == 12u && vr[V - 1] == 0.25f && vr[2 * V] == 0.25f;
    for (int i = 0; i < V; ++i) clean = clean && vr[V + i] == 0.0f;
    CHECK(clean, "clear of stream 1 of 3");
    // the gate over one stream's ring: L = 12 reads entries 5, 6, 7 (slots 5, 6, 7); a threshold <= 0 (or NaN) leaves it open
    const float w[V] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 0.25f, 0.5f, 0.25f};
    memcpy(vr, w, sizeof(w));
    CHECK(!owq::gate_closed(vr, 12u, 0.5f) && owq::gate_closed(vr, 12u, f32(u32(0.5f) + 1u)), "gate at L = 12 with the maximum at the threshold");
    CHECK(!owq::gate_closed(vr, 12u, 0.0f) && !owq::gate_closed(vr, 12u, -1.0f) && !owq::gate_closed(vr, 12u, f32(0x7FC00000u)), "gate with no threshold");
    CHECK(owq::gate_closed(vr, 4u, 0.5f) && owq::gate_closed(vr, 0u, 0.5f) && !owq::gate_closed(vr, 5u, 0.5f), "gate while the window is empty, and on entry 0 alone");
    nv[0] = 12u;
    const owq::Gate on{vr, nv, 0.5f}, off{vr, nullptr, 0.0f};   // (gate off: the counts are not read)
    CHECK(!owq::gate_closed(on, 0) && !owq::gate_closed(off, 0), "gate through the parameter block");
    free(vr); free(nv);
}

// ------------------------------------------------------------------------------------------------------------------ case files
static int run_cases(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    if (!f) { fprintf(stderr, "postproc_check: cannot read %s\n", in_path); return 1; }
    uint32_t n[3];
    if (fread(n, 4, 3, f) != 3) { fprintf(stderr, "postproc_check: %s has no header\n", in_path); fclose(f); return 1; }
    const size_t words = (size_t)n[0] * (5 + D) + (size_t)(n[1] + n[2]) * (2 + V);
    std::vector<uint32_t> in(words);
    const bool whole = fread(in.data(), 4, words, f) == words && fgetc(f) == EOF;
    fclose(f);
    if (!whole) { fprintf(stderr, "postproc_check: %s does not hold %u + %u + %u cases\n", in_path, n[0], n[1], n[2]); return 1; }
    std::vector<uint32_t> out;
    out.reserve((size_t)n[0] * (1 + D) + n[1] + (size_t)n[2] * (1 + V));
    const uint32_t* p = in.data();
    for (uint32_t c = 0; c < n[0]; ++c, p += 5 + D) {
        float ring[D];
        for (int i = 0; i < D; ++i) ring[i] = f32(p[5 + i]);
        out.push_back(u32(rule_once(f32(p[1]), p[0], ring, (int)p[2], f32(p[3]), (int)p[4], (int)(c & 3u))));
        for (int i = 0; i < D; ++i) out.push_back(u32(ring[i]));
    }
    float* vr = (float*)malloc(V * sizeof(float));
    uint32_t* nv = (uint32_t*)malloc(sizeof(uint32_t));
    for (uint32_t c = 0; c < n[1]; ++c, p += 2 + V) {
        for (int i = 0; i < V; ++i) vr[i] = f32(p[2 + i]);
        out.push_back(owq::gate_closed(vr, p[0], f32(p[1])) ? 1u : 0u);
    }
    for (uint32_t c = 0; c < n[2]; ++c, p += 2 + V) {
        for (int i = 0; i < V; ++i) vr[i] = f32(p[2 + i]);
        nv[0] = p[0];
        owq::vad_push(vr, nv, 0, f32(p[1]));
        out.push_back(nv[0]);
        for (int i = 0; i < V; ++i) out.push_back(u32(vr[i]));
    }
    free(vr); free(nv);
    f = fopen(out_path, "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) { fprintf(stderr, "postproc_check: cannot write %s\n", out_path); return 1; }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_cases(argv[1], argv[2]);
    if (argc != 1) { fprintf(stderr, "usage: postproc_check [IN OUT]\n"); return 1; }
    self_checks();
    if (g_bad) return 1;
    printf("done 1\n");
    return 0;
}
