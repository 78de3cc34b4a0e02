// owwhip_pack.h -- the host side of the device weight image: blob parsing, operand-order packers, the f16-split scales, and the phases
// of oww_commit that lay the image out.  Host only and free of HIP: owwhip.hip includes it for the library, and a plain host program
// can include it alone (tests/pack_check.cpp runs every function below under AddressSanitizer / UBSan).  This is the code that
// decides whether the kernels read the right weight: the layouts it writes are documented next to the kernels that read them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "owwhip.h"
#include "owwhip_layout.h"

namespace owp {

inline thread_local std::string g_err;        // oww_last_error

inline int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    try { g_err = buf; } catch (...) {}                // (the message is best effort; the code is what callers branch on)
    return code;
}

// pack [ntaps][cin][cout] for conv_mfma / heads64: out[(ct*KS + s)*64 + lane]
inline void pack_mfma(const float* w, int ntaps, int cin, int cout, std::vector<float>& out) {
    const int nct = (cout + 15) / 16, ks = ntaps * cin / 4;
    out.assign((size_t)nct * ks * 64, 0.f);
    for (int ct = 0; ct < nct; ++ct)
        for (int tap = 0; tap < ntaps; ++tap)
            for (int cb = 0; cb < cin; cb += 8)
                for (int q = 0; q < 2; ++q) {
                    const int s = (tap * cin + cb) / 4 + q;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = lane & 15, j = lane >> 4;
                        const int co = ct * 16 + i, ci = cb + 2 * j + q;
                        out[((size_t)ct * ks + s) * 64 + lane] = co < cout ? w[((size_t)tap * cin + ci) * cout + co] : 0.f;
                    }
                }
}

// register-resident layout (owwhip_rr.h): out[((((oct*ntaps + tap)*ncti + ct)*64 + lane)*4 + e], lane = (i, j):
// weight of input channel 16ct+4j+e and output channel 16oct+i
// a half-filled last input-channel tile (cin % 16 == 8) is consumed in pack_half order: two k-steps, lane (i, j) of
// k-step e' < 2 carrying channel 16ct + 4(j&1) + 2e' + (j>>1); k-steps 2,3 of that block are not executed
inline void pack_rr(const float* w, int ntaps, int cin, int cout, std::vector<float>& out) {
    const int ncti = (cin + 15) / 16, ncto = (cout + 15) / 16;
    const bool half_in = cin % 16 == 8;
    out.assign((size_t)ncto * ntaps * ncti * 64 * 4, 0.f);
    for (int oct = 0; oct < ncto; ++oct)
        for (int tap = 0; tap < ntaps; ++tap)
            for (int ct = 0; ct < ncti; ++ct)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int i = lane & 15, j = lane >> 4;
                        int ci = ct * 16 + 4 * j + e;
                        if (half_in && ct == ncti - 1) ci = e < 2 ? ct * 16 + 4 * (j & 1) + 2 * e + (j >> 1) : cin;
                        const int co = oct * 16 + i;
                        if (ci < cin && co < cout)
                            out[((((size_t)oct * ntaps + tap) * ncti + ct) * 64 + lane) * 4 + e] = w[((size_t)tap * cin + ci) * cout + co];
                    }
}

// the f16 halves of 2^8 * w must stay finite: |w| < 255 (trained linear weights are orders of magnitude below); VAD network
inline bool hx_in_range(const float* w, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!(std::fabs(w[i]) * owh::WSCALE < 65000.f)) return false;
    return true;
}
// heads: the power-of-two exponent e that puts the largest |w| of a matrix at 2^11 .. 2^12 (its f16 halves then carry 22 bits for
// every weight down to 2^-13 of the largest; no weight magnitude is refused); -1000 when a weight is not finite
inline int hx_weight_exp(const float* w, size_t n) {
    float m = 0.f;
    for (size_t i = 0; i < n; ++i) { if (!std::isfinite(w[i])) return -1000; m = std::max(m, std::fabs(w[i])); }
    int e2 = 0;
    if (m > 0.f) std::frexp(m, &e2);                 // m < 2^e2
    return std::min(100, std::max(-100, 12 - e2));
}

// one weight as an f16 (hi, lo) pair: w * mul formed in double, hi = f16(v), lo = f16(v - hi) (22 bits together).
// mul = colmul[cout] for the embedding CNN (folded BatchNorm scale x the layer's activation-scale ratio, see fold_cnn), else 2^8.
struct HxFold {
    const double* colmul = nullptr;      // per output channel; nullptr = owh::WSCALE for every channel
    double absmax = 0.0;                 // largest |w * mul| seen (range check by the caller)
    inline void split(float w, int co, _Float16& hi, _Float16& lo) {
        const double v = (double)w * (colmul ? colmul[co] : (double)owh::WSCALE);
        absmax = std::max(absmax, std::fabs(v));
        hi = (_Float16)v;
        lo = (_Float16)(v - (double)hi);
    }
};

// fp16-split operand order (owwhip_hx.h): blocks [oct][tap][ks][part hi/lo] of 64 lanes x 8 halves; lane (i, g), half q
// <-> weight of the input channel in row 4g + q%4 of channel tile 2ks + q/4 and the output channel in row i of tile oct
// (hx_row_channel)
// rem2 (cin = odd number of FULL channel tiles, stage B's 48): the last k-step in the two-MFMA form of owh::split_dup -- its empty
// half carries the same channels again: block part 0 = (wh | wh), part 1 = (wl | 0)
inline void pack_hx(const float* w, int ntaps, int cin, int cout, std::vector<float>& out, HxFold* fold = nullptr, bool rem2 = false) {
    HxFold dflt; if (!fold) fold = &dflt;
    const int ks_n = ((cin + 15) / 16 + 1) / 2, ncto = (cout + 15) / 16;
    rem2 = rem2 && ((cin + 15) / 16) % 2 == 1 && cin % 16 == 0;
    std::vector<_Float16> hbuf((size_t)ncto * ntaps * ks_n * 2 * 64 * 8, (_Float16)0.f);
    for (int oct = 0; oct < ncto; ++oct)
        for (int tap = 0; tap < ntaps; ++tap)
            for (int ks = 0; ks < ks_n; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int q = 0; q < 8; ++q) {
                        const int i = lane & 15, g = lane >> 4;
                        const bool dup = rem2 && ks == ks_n - 1 && q >= 4;            // the empty half of the remainder k-step
                        const int ci = dup ? hx_row_channel(2 * ks, 4 * g + q % 4, cin) :
                                       (2 * ks + q / 4 < (cin + 15) / 16 ? hx_row_channel(2 * ks + q / 4, 4 * g + q % 4, cin) : -1);
                        const int co = hx_row_channel(oct, i, cout);
                        if (ci < 0 || co < 0) continue;
                        _Float16 hi, lo;
                        fold->split(w[((size_t)tap * cin + ci) * cout + co], co, hi, lo);
                        const size_t blk = (((size_t)oct * ntaps + tap) * ks_n + ks) * 2;
                        hbuf[(blk * 64 + lane) * 8 + q] = hi;
                        hbuf[((blk + 1) * 64 + lane) * 8 + q] = dup ? (_Float16)0.f : lo;
                    }
    out.assign(hbuf.size() / 2, 0.f);
    memcpy(out.data(), hbuf.data(), hbuf.size() * sizeof(_Float16));
}
// K-merged 3x1 (time) layer of a stage with an odd number of channel tiles (owh::conv_time_hxm): per output tile the blocks
// [tap][full k-step][part], then [merged k-step][part]; merged k-step mk, lane (i, g), half q: pair index pi = 4 mk + q/2 carries
// tap pi / NPR, pair v = pi % NPR of the remainder tile, i.e. its row 4g + 2v + q%2
inline void pack_hx_tm(const float* w, int cin, int cout, std::vector<float>& out, HxFold* fold) {
    const int ncti = (cin + 15) / 16, ncto = (cout + 15) / 16;
    const bool half = cin % 16 == 8;
    const int ksf = ncti / 2, npr = half ? 1 : 2, nmk = (3 * npr + 3) / 4, nb = (3 * ksf + nmk) * 2;
    std::vector<_Float16> hbuf((size_t)ncto * nb * 64 * 8, (_Float16)0.f);
    auto put = [&](size_t blk, int lane, int q, int tap, int ci, int co) {
        if (ci < 0 || co < 0) return;
        _Float16 hi, lo;
        fold->split(w[((size_t)tap * cin + ci) * cout + co], co, hi, lo);
        hbuf[(blk * 64 + lane) * 8 + q] = hi;
        hbuf[((blk + 1) * 64 + lane) * 8 + q] = lo;
    };
    for (int oct = 0; oct < ncto; ++oct)
        for (int lane = 0; lane < 64; ++lane)
            for (int q = 0; q < 8; ++q) {
                const int i = lane & 15, g = lane >> 4, co = hx_row_channel(oct, i, cout);
                for (int tap = 0; tap < 3; ++tap)
                    for (int ks = 0; ks < ksf; ++ks)
                        put(((size_t)oct * nb) + (tap * ksf + ks) * 2, lane, q, tap, hx_row_channel(2 * ks + q / 4, 4 * g + q % 4, cin), co);
                for (int mk = 0; mk < nmk; ++mk) {
                    const int pi = 4 * mk + q / 2;
                    if (pi >= 3 * npr) continue;
                    const int tap = pi / npr, v = pi % npr;
                    put(((size_t)oct * nb) + (3 * ksf + mk) * 2, lane, q, tap, hx_row_channel(ncti - 1, 4 * g + 2 * v + q % 2, cin), co);
                }
            }
    out.assign(hbuf.size() / 2, 0.f);
    memcpy(out.data(), hbuf.data(), hbuf.size() * sizeof(_Float16));
}
// per-channel array (folded BatchNorm scale / shift) in the row order of the f16-split tiles, zero in padding rows
inline void pad_hx_rows(const float* v, int C, float mul, std::vector<float>& out) {
    const int nct = (C + 15) / 16;
    out.assign((size_t)nct * 16, 0.f);
    for (int t = 0; t < nct; ++t)
        for (int r = 0; r < 16; ++r) { const int c = hx_row_channel(t, r, C); if (c >= 0) out[t * 16 + r] = v[c] * mul; }
}
// heads layer 1 (owh::heads_hx_kernel): k-step major [K/32][NH/16][part][64][8]; lane (i, g), half q <-> input 32ks + 8g + q
inline void pack_hx_w1(const float* wcat /*[K][NH]*/, int K, int NH, const double* colmul /*[NH]*/, std::vector<float>& out) {
    const int nks = K / 32, nct = NH / 16;
    std::vector<_Float16> hbuf((size_t)nks * nct * 2 * 64 * 8, (_Float16)0.f);
    for (int ks = 0; ks < nks; ++ks)
        for (int ct = 0; ct < nct; ++ct)
            for (int lane = 0; lane < 64; ++lane)
                for (int q = 0; q < 8; ++q) {
                    const int i = lane & 15, g = lane >> 4;
                    const double v = (double)wcat[(size_t)(32 * ks + 8 * g + q) * NH + 16 * ct + i] * colmul[16 * ct + i];
                    const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (double)hi);
                    const size_t blk = ((size_t)ks * nct + ct) * 2;
                    hbuf[(blk * 64 + lane) * 8 + q] = hi;
                    hbuf[((blk + 1) * 64 + lane) * 8 + q] = lo;
                }
    out.assign(hbuf.size() / 2, 0.f);
    memcpy(out.data(), hbuf.data(), hbuf.size() * sizeof(_Float16));
}
// conv0 (3x3, one input channel, K = 9) in the K-folded form of owh::hstageA_stream: the three products of the f16 split share ONE
// k-step -- k-slot 8g + q of lane (i, g): slots 0..8 = wh[tap] (against xh), 9..17 = wl[tap] (against xh), 18..26 = wh[tap] (against
// xl), 27..31 = 0.  One 1 KB block per output-channel tile.
inline void pack_hx_conv0(const float* w /*[9][24]*/, std::vector<float>& out, HxFold* fold) {
    std::vector<_Float16> hbuf((size_t)2 * 64 * 8, (_Float16)0.f);
    for (int oct = 0; oct < 2; ++oct)
        for (int lane = 0; lane < 64; ++lane)
            for (int q = 0; q < 8; ++q) {
                const int i = lane & 15, g = lane >> 4, slot = 8 * g + q, co = hx_row_channel(oct, i, 24);
                if (slot >= 27 || co < 0) continue;
                _Float16 hi, lo;
                fold->split(w[(slot % 9) * 24 + co], co, hi, lo);
                hbuf[((size_t)oct * 64 + lane) * 8 + q] = (slot / 9 == 1) ? lo : hi;
            }
    out.assign(hbuf.size() / 2, 0.f);
    memcpy(out.data(), hbuf.data(), hbuf.size() * sizeof(_Float16));
}

// stage A's two 24 -> 24 layers (owh::hstageA_stream): channel tile 0 as in pack_hx -- blocks [tap][part] -- and the HALF tile (channels
// 16..23 in rows 4j + e, e < 2) with a second tap stacked into its free rows 4j + e, e >= 2:
//   conv1 (1x3): blocks (W2 | W0), (W1 | 0), (W0 | W2): the side chain of a parity tile rides in the main chain's registers 2, 3;
//   conv2 (3x1): blocks (W_i | W_{i-1}) for input row i = 0..3 of [history 0, history 1, row 2q, row 2q+1]: registers 0, 1 accumulate
//                output row 2q, registers 2, 3 output row 2q+1.
inline void pack_hx_stage_a(const float* w /*[3][24][24]*/, int layer, std::vector<float>& out, HxFold* fold) {
    const int nblk = layer == 1 ? 12 : 14;
    std::vector<_Float16> hbuf((size_t)nblk * 64 * 8, (_Float16)0.f);
    auto put = [&](int blk, int lane, int q, int tap, int ci, int co) {
        if (tap < 0 || tap > 2 || ci < 0 || co < 0) return;
        _Float16 hi, lo;
        fold->split(w[((size_t)tap * 24 + ci) * 24 + co], co, hi, lo);
        hbuf[((size_t)blk * 64 + lane) * 8 + q] = hi;
        hbuf[((size_t)(blk + 1) * 64 + lane) * 8 + q] = lo;
    };
    for (int lane = 0; lane < 64; ++lane)
        for (int q = 0; q < 8; ++q) {
            const int i = lane & 15, g = lane >> 4, ci = hx_row_channel(q / 4, 4 * g + q % 4, 24);
            for (int tap = 0; tap < 3; ++tap) put(tap * 2, lane, q, tap, ci, i);                       // channel tile 0: output channel i
            const int j = i >> 2, e = i & 3, co = 16 + 2 * j + (e & 1);
            if (layer == 1) {
                const int lo_tap[3] = {2, 1, 0}, hi_tap[3] = {0, -1, 2};
                for (int v = 0; v < 3; ++v) put(6 + v * 2, lane, q, e < 2 ? lo_tap[v] : hi_tap[v], ci, co);
            } else {
                for (int r = 0; r < 4; ++r) put(6 + r * 2, lane, q, e < 2 ? r : r - 1, ci, co);
            }
        }
    out.assign(hbuf.size() / 2, 0.f);
    memcpy(out.data(), hbuf.data(), hbuf.size() * sizeof(_Float16));
}

struct HostBuf {                      // host image of the device weight buffer (256-byte aligned pieces)
    std::vector<float> data;
    size_t add(const float* p, size_t n) {
        const size_t off = (data.size() + 63) / 64 * 64;
        data.resize(off + n);
        if (p) memcpy(data.data() + off, p, n * sizeof(float));
        return off;
    }
    size_t add(const std::vector<float>& v) { return add(v.data(), v.size()); }
};

struct NetHost {
    int hidden, n_out, has_ln, T, final_act, head, role, out_col;
    int n_blocks;                     // hidden blocks behind the first layer (train.py:73: Net's n_blocks; 1 in every released model)
    const float *w1, *b1, *ln1g, *ln1b, *w2, *b2, *ln2g, *ln2b, *w3, *b3;   // into the owning head blob (w2 .. ln2b: block 0)
    const float* blocks;              // the n_blocks blocks back to back: w[H][H] b[H] (g[H] be[H])
    const float* rnn = nullptr;       // model_type "rnn" (kind 3): the head's blob (owk::heads_rnn_kernel); its size in rnn_floats
    size_t rnn_floats = 0;
};
struct HeadHost {
    int kind, T, hidden, n_out, has_ln, n_blocks;
    std::vector<float> blob;
    int out_col;
};
// A fast group: nets of one T that share a launch of the MFMA head kernels (pack_head_groups sorts the heads into them)
struct HeadGroup {
    int T, NH, n_nets;
    std::vector<int> nets;            // indices into all nets
    // fp16-split fast path: ht hidden tiles of 16 units per net.  4: nets of up to 64 units, zero-padded (pack_hx_net).  8: the wide
    // form (owh::heads_wide_tail: nets of up to 128 hidden units / 8 outputs, sigmoid or ReLU + softmax -- the multiclass `timer`
    // model), at most two nets per launch
    int ht = 4;
};

// A dense head net inside its blob: w1[T * 96][H] b1 (ln1g ln1b) | n_blocks x (w[H][H] b (g be)) | w3[H][O] b3.  Fills the net's shape
// and pointers (LayerNorm arrays stay null without LayerNorm; w2 .. ln2b name block 0: what the MFMA head kernels read); returns the end.
inline const float* parse_dense_net(const float* q, int T, int hidden, int n_out, int has_ln, int n_blocks, NetHost& n) {
    const size_t K = (size_t)T * 96, H = hidden, O = n_out;
    n.T = T; n.hidden = hidden; n.n_out = n_out; n.has_ln = has_ln; n.n_blocks = n_blocks;
    n.w1 = q; q += K * H; n.b1 = q; q += H;
    if (has_ln) { n.ln1g = q; q += H; n.ln1b = q; q += H; }
    n.blocks = q;
    if (n_blocks > 0) { n.w2 = q; n.b2 = q + H * H; }
    if (n_blocks > 0 && has_ln) { n.ln2g = n.b2 + H; n.ln2b = n.ln2g + H; }
    q += (size_t)n_blocks * (H * H + H + (has_ln ? 2 * H : 0));
    n.w3 = q; q += H * O; n.b3 = q; q += O;
    return q;
}

// ---- one net in the form of the fp16-split heads kernels (heads_hx_kernel, heads_bank_kernel), fixed heads and bank heads alike: ht
// hidden tiles (4: up to 64 hidden units, one sigmoid output; 8: the wide form), HP = 16 ht units of which those beyond n.hidden are
// identically zero and left out of the LayerNorm statistics (owh::HeadHxNet::hidden; the reference's training pipeline defaults to 32
// units: examples/custom_model.yml:89).  Every matrix on its own power-of-two scale (hx_weight_exp), undone on the fp32 accumulators.
struct HxNetPack {
    int e1 = 0, e2 = 0, e3 = 0;           // scales of w1 / w2 / w3 (wide form)
    int eh = 0;                           // narrow form: scale of the hidden vector between layer 1 and layer 2 (hx_hidden_exp)
    size_t w2 = 0, w3 = 0, pad = 0;       // where pack_hx_net put the pieces, floats from the start of the image
};

// Up to 64 windows of the commit's probe embeddings (probe_emb [nb * 16 frames][32 probes][96]) as a head of T rows sees them: window w
// belongs to probe w % 32 of batch w / 32 and ends on the batch's last frame; rows before the batch's first frame stay 0.  What
// oww_bank_add's self-test scores and what hx_hidden_exp measures.  -> number of windows (>= 1; all zero without probes)
inline int probe_windows(const std::vector<float>& probe_emb, int probe_nb, int T, std::vector<float>& win) {
    const int NP = 32, CT = 16;
    const int B = std::min(64, std::max(1, probe_nb) * NP);      // (64 windows: ~10 ms of float64 per head)
    win.assign((size_t)B * T * 96, 0.f);
    for (int w = 0; w < B && !probe_emb.empty(); ++w) {
        const int bt0 = (w / NP) * CT, pr = w % NP;
        for (int r = 0; r < T; ++r) {
            const int fr = CT - T + r;
            if (fr < 0) continue;
            memcpy(&win[((size_t)w * T + r) * 96], &probe_emb[(((size_t)bt0 + fr) * NP + pr) * 96], 96 * sizeof(float));
        }
    }
    return B;
}

// The narrow form (ht 4) hands its hidden vector relu(ln1(W1 x + b1)) to the second GEMM through the f16 hi / lo split with no scale
// applied in the kernel, and nothing in a net bounds that vector: ln1's gamma / beta set its magnitude, or W1, b1 and the audio where
// there is no LayerNorm.  Units of order 1e-4 lose the low halves of their split to the f16 subnormal grid, units beyond 65504 leave
// the range (tests/test_head_regimes.py: ln1_cold, noln_cold, noln_hot).  ReLU commutes with a positive power of two, so the scale is
// folded into the weights on the host: 2^eh into ln1's gamma and beta (without LayerNorm: into u1 and b1), 2^-eh into u2 -- exact,
// and the kernels do not change.  eh puts the largest hidden unit over the probe windows at 2^9 .. 2^10, where oww_commit puts the
// largest probe embedding (hx_efeat): the same factor 64 below the f16 overflow.  float64 on the host, once per net; 0 without probes
// or when no unit is ever positive.  The wide form scales each stream's vector in the kernel (owh::scale_own) and needs none.
inline int hx_hidden_exp(const NetHost& n, const std::vector<float>& probe_emb, int probe_nb) {
    if (probe_emb.empty()) return 0;
    const size_t K = (size_t)n.T * 96, H = n.hidden;
    std::vector<float> win;
    const int B = probe_windows(probe_emb, probe_nb, n.T, win);
    std::vector<double> a(H);
    double mx = 0.0;
    for (int w = 0; w < B; ++w) {
        const float* x = &win[(size_t)w * K];
        for (size_t j = 0; j < H; ++j) a[j] = n.b1[j];
        for (size_t k = 0; k < K; ++k) {
            const double xv = x[k];
            const float* wr = n.w1 + k * H;
            for (size_t j = 0; j < H; ++j) a[j] += xv * wr[j];
        }
        if (n.has_ln) {
            double mu = 0.0, var = 0.0;
            for (size_t j = 0; j < H; ++j) mu += a[j];
            mu /= (double)H;
            for (size_t j = 0; j < H; ++j) var += (a[j] - mu) * (a[j] - mu);
            const double rs = 1.0 / std::sqrt(var / (double)H + 1e-5);
            for (size_t j = 0; j < H; ++j) a[j] = (a[j] - mu) * rs * n.ln1g[j] + n.ln1b[j];
        }
        for (size_t j = 0; j < H; ++j) if (a[j] > mx) mx = a[j];
    }
    if (!(mx > 0.0) || !std::isfinite(mx)) return 0;
    int e2 = 0;
    std::frexp(mx, &e2);                                   // mx = f 2^e2, f in [0.5, 1)
    return std::min(60, std::max(-60, 10 - e2));
}

// the scales of a net's matrices and, narrow form, of its hidden vector; false when a weight is not finite
inline bool hx_net_scales(const NetHost& n, int ht, HxNetPack& p, const std::vector<float>& probe_emb, int probe_nb) {
    const size_t K = (size_t)n.T * 96, H = n.hidden;
    p.e1 = hx_weight_exp(n.w1, K * H); p.e2 = hx_weight_exp(n.w2, H * H); p.e3 = ht == 8 ? hx_weight_exp(n.w3, H * n.n_out) : 0;
    if (p.e1 == -1000 || p.e2 == -1000 || p.e3 == -1000) return false;
    p.eh = ht == 4 ? hx_hidden_exp(n, probe_emb, probe_nb) : 0;
    return true;
}

// First layer: the net's w1[K][H] into columns [c0, c0 + H) of a zeroed [K][NH] matrix (its columns up to c0 + HP stay zero), 2^e1 as
// the multiplier of its HP columns.  The caller packs the matrix (pack_hx_w1): a fixed group its nets side by side, a bank head its own.
inline void place_w1(const NetHost& n, int c0, int HP, int NH, int e1, std::vector<float>& wcat, std::vector<double>& colmul) {
    const size_t K = (size_t)n.T * 96, H = n.hidden;
    for (size_t k = 0; k < K; ++k) memcpy(&wcat[k * NH + c0], n.w1 + k * H, H * sizeof(float));
    for (int c = 0; c < HP; ++c) colmul[c0 + c] = std::ldexp(1.0, e1);
}

// Everything behind the first layer, appended to the image in this order: w2 zero-padded to [HP][HP]; in the wide form the output layer
// as a third split matrix [HP][16] (outputs n_out .. 15 zero); the pad block -- b1, ln1 g / b, b2, ln2 g / b and, in the narrow form, w3
// at a stride of HP floats, then b3: 16 floats in the wide form, 4 in the narrow form where b3_in_pad (bank heads), none otherwise
// (the kernel reads a fixed narrow net's b3 from the net's natural array).  Narrow form: 2^eh folded into ln1 g / b, or into b1.
inline void pack_hx_net(const NetHost& n, int ht, bool b3_in_pad, HostBuf& hb, HxNetPack& p) {
    const size_t HP = 16 * (size_t)ht, H = n.hidden, O = n.n_out;
    std::vector<float> pk;
    auto add_split = [&](const float* w, size_t cols, size_t CP, int e) {      // w[H][cols] inside a zero [HP][CP], times 2^e
        std::vector<double> cm(CP, std::ldexp(1.0, e));
        HxFold fold; fold.colmul = cm.data();
        std::vector<float> wp(HP * CP, 0.f);
        for (size_t i = 0; i < H; ++i) memcpy(&wp[i * CP], w + i * cols, cols * sizeof(float));
        pack_hx(wp.data(), 1, (int)HP, (int)CP, pk, &fold);
        return hb.add(pk);
    };
    p.w2 = add_split(n.w2, H, HP, p.e2);
    if (ht == 8) p.w3 = add_split(n.w3, O, 16, p.e3);
    const size_t n_arr = ht == 8 ? 6 : 7, n_b3 = ht == 8 ? 16 : b3_in_pad ? 4 : 0;
    std::vector<float> pad(n_arr * HP + n_b3, 0.f);
    const float* src[7] = {n.b1, n.ln1g, n.ln1b, n.b2, n.ln2g, n.ln2b, n.w3};
    for (size_t a = 0; a < n_arr; ++a) if (src[a]) memcpy(&pad[a * HP], src[a], H * sizeof(float));
    if (p.eh != 0) {                      // the hidden vector's scale (hx_hidden_exp): ln1 g and b, or b1 (with u1: make_hx_net)
        if (n.has_ln) for (size_t i = HP; i < 3 * HP; ++i) pad[i] = std::ldexp(pad[i], p.eh);
        else for (size_t i = 0; i < HP; ++i) pad[i] = std::ldexp(pad[i], p.eh);
    }
    if (n_b3) memcpy(&pad[n_arr * HP], n.b3, O * sizeof(float));
    p.pad = hb.add(pad);
}

// float64 evaluation of a binary one-block net on one window x[T][96]: the bank self-test's reference
inline double bank_eval_f64(const NetHost& n, const float* x) {
    const size_t K = (size_t)n.T * 96;
    const int H = n.hidden;
    std::vector<double> a(H), z(H);
    auto ln_relu = [&](std::vector<double>& v, const float* g, const float* be) {
        if (n.has_ln) {
            double mu = 0.0, var = 0.0;
            for (int i = 0; i < H; ++i) mu += v[i];
            mu /= H;
            for (int i = 0; i < H; ++i) var += (v[i] - mu) * (v[i] - mu);
            const double rs = 1.0 / std::sqrt(var / H + 1e-5);
            for (int i = 0; i < H; ++i) v[i] = (v[i] - mu) * rs * g[i] + be[i];
        }
        for (int i = 0; i < H; ++i) v[i] = std::max(v[i], 0.0);
    };
    for (int i = 0; i < H; ++i) a[i] = n.b1[i];
    for (size_t k = 0; k < K; ++k) for (int i = 0; i < H; ++i) a[i] += (double)x[k] * n.w1[k * H + i];
    ln_relu(a, n.ln1g, n.ln1b);
    for (int i = 0; i < H; ++i) z[i] = n.b2[i];
    for (int k = 0; k < H; ++k) for (int i = 0; i < H; ++i) z[i] += a[k] * n.w2[(size_t)k * H + i];
    ln_relu(z, n.ln2g, n.ln2b);
    double o = n.b3[0];
    for (int i = 0; i < H; ++i) o += z[i] * n.w3[i];
    return 1.0 / (1.0 + std::exp(-o));
}

// ---- blob parsing (oww_load_mel / oww_load_embedding / oww_add_head / oww_bank_add / oww_load_vad): size, header and finiteness
// checks; `out` is written only when the blob is accepted
inline int parse_mel_blob(const void* blob, size_t nbytes, std::vector<float>& out) {
    const size_t want = (400 + 32 + 32 * 16) * 4;
    if (nbytes != want) return fail(OWW_EINVAL, "oww_load_mel: blob is %zu bytes, expected %zu", nbytes, want);
    out.assign((const float*)blob, (const float*)blob + want / 4);
    return OWW_OK;
}

inline int parse_embedding_blob(const void* blob, size_t nbytes, std::vector<float>& out) {
    size_t want = 0;
    for (int l = 0; l < 20; ++l) {
        want += (size_t)kLayers[l].kh * kLayers[l].kw * kLayers[l].cin * kLayers[l].cout;
        if (l < 19) want += 2 * (size_t)kLayers[l].cout;
    }
    if (nbytes != want * 4) return fail(OWW_EINVAL, "oww_load_embedding: blob is %zu bytes, expected %zu", nbytes, want * 4);
    // (a NaN weight would not fail later: the max()-based activation swallows it, in every kernel family)
    for (size_t i = 0; i < want; ++i)
        if (!std::isfinite(((const float*)blob)[i])) return fail(OWW_EINVAL, "oww_load_embedding: weights are not finite (float %zu of the blob)", i);
    out.assign((const float*)blob, (const float*)blob + want);
    return OWW_OK;
}

// floats of a dense head's blob behind its header: per net w1 b1 (ln1) | n_blocks x (w b (ln)) | w3 b3; gated heads have two nets
inline size_t dense_head_floats(int kind, int T, int hidden, int n_out, int has_ln, int n_blocks) {
    const size_t in = (size_t)T * 96, H = hidden, O = n_out;
    const size_t per_net = in * H + H + (has_ln ? 2 * H : 0) + (size_t)n_blocks * (H * H + H + (has_ln ? 2 * H : 0)) + H * O + O;
    return per_net * (kind == 1 ? 2 : 1);
}

// fn: the entry point the messages name.  t_max: 120 for a fixed head; oww_bank_add passes the handle's feature ring.
inline int parse_head_blob(const char* fn, const void* blob, size_t nbytes, int t_max, HeadHost& out) {
    if (nbytes < 32) return fail(OWW_EINVAL, "%s: bad argument", fn);
    const int32_t* hdr = (const int32_t*)blob;
    HeadHost hh{};
    hh.kind = hdr[0]; hh.T = hdr[1]; hh.hidden = hdr[2]; hh.n_out = hdr[3]; hh.has_ln = hdr[4];
    hh.n_blocks = 1 + hdr[5];                  // (hdr[5] = hidden blocks beyond the one every released model has; -1 = none)
    size_t want = 0;
    if (hh.kind == 3) {                        // train.py:85-98: 2-layer bidirectional LSTM(64) + Linear(128, n_out)
        using owk::RNN_H; using owk::RNN_TMAX;
        if (hh.T < 1 || hh.T > RNN_TMAX || hh.hidden != RNN_H || hh.n_out < 1 || hh.n_out > 8 || hh.has_ln || hdr[5] != 0)
            return fail(OWW_EINVAL, "%s: bad rnn header T=%d (<= %d) hidden=%d (= %d) n_out=%d", fn, hh.T, RNN_TMAX, hh.hidden, RNN_H, hh.n_out);
        want = 2 * ((size_t)(96 + RNN_H) * 256 + 256) + 2 * ((size_t)(128 + RNN_H) * 256 + 256) + (size_t)128 * hh.n_out + hh.n_out;
        if (nbytes != 32 + want * 4) return fail(OWW_EINVAL, "%s: rnn blob is %zu bytes, expected %zu", fn, nbytes, 32 + want * 4);
    } else {
        if (hh.kind < 0 || hh.kind > 2 || hh.T < 1 || hh.T > t_max || hh.hidden < 1 || hh.hidden > 512 || hh.n_out < 1 || hh.n_out > 8 ||
            hh.n_blocks < 0 || hh.n_blocks > OWW_MAX_HEAD_BLOCKS)
            return fail(OWW_EINVAL, "%s: bad header kind=%d T=%d hidden=%d n_out=%d blocks=%d", fn, hh.kind, hh.T, hh.hidden, hh.n_out, hh.n_blocks);
        want = dense_head_floats(hh.kind, hh.T, hh.hidden, hh.n_out, hh.has_ln, hh.n_blocks);
        if (nbytes != 32 + want * 4) return fail(OWW_EINVAL, "%s: blob is %zu bytes, expected %zu", fn, nbytes, 32 + want * 4);
    }
    const float* q = (const float*)((const char*)blob + 32);
    for (size_t i = 0; i < want; ++i)
        if (!std::isfinite(q[i])) return fail(OWW_EINVAL, "%s: head weights are not finite (float %zu of the blob)", fn, i);
    hh.blob.assign(q, q + want);
    out = std::move(hh);
    return OWW_OK;
}

inline int parse_vad_blob(const void* blob, size_t nbytes, std::vector<float>& out) {
    const size_t want = 32 + vad_blob_floats() * 4;
    if (nbytes != want) return fail(OWW_EINVAL, "oww_load_vad: blob is %zu bytes, expected %zu", nbytes, want);
    const int32_t* hdr = (const int32_t*)blob;
    if (hdr[0] != 1 || hdr[1] != 256 || hdr[2] != 64 || hdr[3] != 128 || hdr[4] != 64)
        return fail(OWW_EINVAL, "oww_load_vad: unsupported geometry (version %d, n_fft %d, hop %d, bins %d, hidden %d)", hdr[0], hdr[1], hdr[2], hdr[3], hdr[4]);
    out.assign((const float*)((const char*)blob + 32), (const float*)((const char*)blob + nbytes));
    return OWW_OK;
}

// ---- f16-split family: the output of layer l is carried multiplied by 2^hx_e[l], its input arrives multiplied by 2^hx_ein[l]
// (owwhip_hx.h act1).  Inside a stage hx_ein[l] = hx_e[l - 1]; the pooled hand-over between two stages (and the pooled input of
// conv19) is re-scaled by 2^hx_xexp[stage], the embedding by 2^-hx_e[19] when it is stored; the features enter the heads' first GEMM
// multiplied by 2^hx_efeat (largest probe |embedding| at 2^9..2^10).
struct HxLadder { int hx_e[20] = {}, hx_ein[20] = {}, hx_xexp[5] = {}, hx_efeat = 0; };

// Scale ladder from every layer's largest |activation| in the calibration run (calibrate_hx) and the embedding blob.
// acc = sum W' X needs no multiply after it only if W' = s w 2^(e_out - e_in), so the weights' magnitude is
// pinned by the exponent step of the layer; their low halves stay precise (abs error 2^-25 against sums of magnitude
// 2^(e_out) |y|) when that step is >= ~2.  Inside a stage the activation maxima therefore climb 2^3 (pooled input) ->
// 2^5 -> 2^7 -> 2^9 -> 2^11 (a factor 32 below the f16 overflow for the loudest probe) and the pooled hand-over, which
// is multiplied once per stored value anyway, brings the next stage's input back to 2^3.
inline void hx_ladder(const float absmax[20], const std::vector<float>& emb_blob, HxLadder& o) {
    auto ex = [&](int l) { int e2 = 0; if (absmax[l] > 0.f) std::frexp(absmax[l], &e2); return e2; };   // max < 2^ex
    auto cl = [](int e2) { return std::min(100, std::max(-100, e2)); };
    const int first[5] = {0, 3, 7, 11, 15};
    for (int st = 0; st < 5; ++st) {
        const int n = st == 0 ? 3 : 4;
        for (int i = 0; i < n; ++i) {
            const int l = first[st] + i;
            o.hx_e[l] = cl((st == 0 ? 7 : 5) + 2 * i - ex(l));
            o.hx_ein[l] = i == 0 ? (st == 0 ? 0 : cl(3 - ex(l - 1))) : o.hx_e[l - 1];     // (max-pooling keeps the maximum)
        }
    }
    o.hx_ein[19] = cl(3 - ex(18));
    // conv19: no BatchNorm, no activation, and its accumulator is un-scaled in fp32 when the embedding is stored -- nothing pins its
    // output range, so the exponent step is chosen for the WEIGHTS: the largest |w| 2^step at 2^11..2^12 (a network whose last
    // layer is 1e-4 x weaker keeps 22 bits per weight: tests/test_weight_regimes.py, tiny_embedding)
    {
        const float* q = emb_blob.data();
        for (int l = 0; l < 19; ++l) q += (size_t)kLayers[l].kh * kLayers[l].kw * kLayers[l].cin * kLayers[l].cout + 2 * kLayers[l].cout;
        const int step = hx_weight_exp(q, (size_t)kLayers[19].kh * kLayers[19].kw * kLayers[19].cin * kLayers[19].cout);
        o.hx_e[19] = cl(o.hx_ein[19] + (step == -1000 ? 2 : step));
    }
    o.hx_efeat = cl(10 - ex(19));                          // the heads' GEMM takes the (true-unit) feature ring at this scale
    for (int st = 0; st < 5; ++st) {
        const int last = st == 0 ? 2 : first[st] + 3, nxt = last + 1;
        o.hx_xexp[st] = o.hx_ein[nxt] - o.hx_e[last];
    }
}

// What the image phases read: the weights as loaded, the kernel family, the f16-split scales and the commit's probe embeddings.
struct PackIn : HxLadder {
    std::vector<float> mel_blob, emb_blob, vad_blob;     // host side weights as loaded
    std::vector<HeadHost> heads;
    std::vector<NetHost> nets;                           // build_nets
    std::vector<std::pair<int, int>> head_nets;          // [begin,end) into nets per head
    bool mfma = true;
    bool rr = true;                   // register-resident CNN kernels (owwhip_rr.h); false = LDS-tiled kernels (MFMA or VALU)
    bool hx = false;                  // fp16-split form of the register-resident kernels (owwhip_hx.h); shares rr's layouts
    std::vector<float> probe_emb;     // oww_commit's fp32 probe embeddings [nb * 16][32][96]: hx_hidden_exp, oww_bank_add's self-test
    int probe_nb = 0;
    int feature_ring = 0;             // oww_config::feature_ring
    bool no_wide_heads = false;       // OWW_NO_WIDE_HEADS: A/B switch, wide heads go to the generic kernel
};

// ---- oww_commit, phase by phase ------------------------------------------------------------------------------------------------------
// Where the pack_* phases put every piece of the device weight image (floats from its start); bind_weights turns them into pointers.
struct WeightOff {
    size_t hann = 0, start = 0, taps = 0, meloff = 0, meldst = 0;
    size_t conv[20] = {}, scale[20] = {}, shift[20] = {};
    struct Net { size_t w1, b1, ln1g, ln1b, w2, b2, ln2g, ln2b, w3, b3, w2pk, blocks, rnn; };
    std::vector<Net> net;                       // natural arrays of every net
    struct Group { size_t w1pk = 0, b1cat = 0, w1hx = 0; std::vector<HxNetPack> net; };
    std::vector<Group> group;                   // per HeadGroup
    size_t vhann = 0, vencw = 0, vencb = 0, vlw = 0, vlb = 0, vwd = 0;
};

// heads -> nets, label columns, feature-ring depth
inline int build_nets(PackIn& in, int& NL, int& TR, int& generic_hmax) {
    in.nets.clear(); in.head_nets.clear();
    int col = 0, maxT = 16, hmax = 1;
    for (size_t hi = 0; hi < in.heads.size(); ++hi) {
        HeadHost& hh = in.heads[hi];
        hh.out_col = col;
        const float* q = hh.blob.data();
        const int begin = (int)in.nets.size();
        for (int r = 0; r < (hh.kind == 1 ? 2 : 1); ++r) {                   // (gated heads: two nets)
            NetHost n{};
            n.head = (int)hi; n.role = r; n.out_col = col;
            if (hh.kind == 3) {                                              // recurrent head: one net, its blob as a whole
                n.hidden = hh.hidden; n.n_out = hh.n_out; n.T = hh.T; n.final_act = hh.n_out == 1 ? 0 : 1;
                n.rnn = q; n.rnn_floats = hh.blob.size();
            } else {
                q = parse_dense_net(q, hh.T, hh.hidden, hh.n_out, hh.has_ln, hh.n_blocks, n);
                n.final_act = hh.kind == 2 ? 1 : 0;
            }
            in.nets.push_back(n);
        }
        in.head_nets.push_back({begin, (int)in.nets.size()});
        col += hh.n_out;
        maxT = std::max(maxT, hh.T);
        hmax = std::max(hmax, hh.hidden);
    }
    NL = col;
    if (NL > OWW_MAX_LABELS) return fail(OWW_EINVAL, "too many labels (%d)", NL);
    TR = in.feature_ring > 0 ? std::max(in.feature_ring, maxT) : maxT;
    generic_hmax = hmax;
    return 0;
}

// The mel front end's tables.  Fused front end: the sparse mel taps read a COMPACT copy of each frame's power row -- one segment per mel
// bin, [first tap .. last non-zero tap] -- whose segment starts have pairwise different residues mod 32, so that the 32 lanes of a tap
// read hit 32 different LDS banks (the plain power row gave three bins per bank for every tap: most of the launch's bank conflicts).
// Every power bin belongs to at most two triangular filters, hence two destinations per bin (mel_dst: lo / hi 16 bits; kMelJunk = none).
inline int pack_mel_tables(const PackIn& in, HostBuf& hb, WeightOff& o) {
    o.hann = hb.add(in.mel_blob.data(), 400);
    o.start = hb.add(in.mel_blob.data() + 400, 32);          // int32 bit patterns
    o.taps = hb.add(in.mel_blob.data() + 432, 512);
    constexpr int kMelTable = 250, kMelJunk = 250;           // floats of a frame's table; bins without a second filter store here
    const int32_t* start = reinterpret_cast<const int32_t*>(in.mel_blob.data() + 400);
    const float* taps = in.mel_blob.data() + 432;
    int nz[32], first[32];
    for (int m = 0; m < 32; ++m) {
        nz[m] = 0;
        for (int t = 0; t < 16; ++t) if (taps[m * 16 + t] != 0.f) nz[m] = t + 1;
        first[m] = start[m] - 2;                              // power-row index of tap 0 (the kernels keep FFT bins 2..121)
    }
    int off[32], best[32], best_end = 1 << 30;
    uint64_t st = 0x9E3779B97F4A7C15ull;
    for (int it = 0; it < 20000 && best_end > kMelTable; ++it) {                // randomised first-fit; a few hundred tries are enough
        int order[32];
        for (int i = 0; i < 32; ++i) order[i] = i;
        for (int i = 31; i > 0; --i) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; std::swap(order[i], order[st % (uint64_t)(i + 1)]); }
        unsigned used = 0; int cur = 0, end = 0;
        for (int i = 0; i < 32; ++i) {
            const int m = order[i];
            int p = cur;
            while (used >> (p & 31) & 1u) ++p;
            used |= 1u << (p & 31); off[m] = p; cur = p + nz[m];
            end = std::max(end, p + 16);                      // a lane reads 16 taps from its start
        }
        if (end < best_end) { best_end = end; memcpy(best, off, sizeof off); }
    }
    if (best_end > kMelTable) {                               // (cannot happen for a 32-filter bank of <= 16 taps; plain prefix layout)
        int cur = 0;
        for (int m = 0; m < 32; ++m) { best[m] = cur; cur += nz[m]; }
        if (cur + 16 > kMelTable) return fail(OWW_EINVAL, "oww_commit: the mel filter bank has more than %d taps", kMelTable - 16);
    }
    std::vector<float> dst(128, 0.f);
    for (int i = 0; i < 120; ++i) {
        uint32_t d[2] = {kMelJunk, kMelJunk}; int n = 0;
        for (int m = 0; m < 32; ++m) {
            const int t = i - first[m];
            if (t >= 0 && t < nz[m] && taps[m * 16 + t] != 0.f) {
                if (n == 2) return fail(OWW_EINVAL, "oww_commit: FFT bin %d feeds more than two mel filters (not a triangular filter bank)", i + 2);
                d[n++] = (uint32_t)(best[m] + t);
            }
        }
        const uint32_t packed = d[0] | (d[1] << 16);
        memcpy(&dst[i], &packed, 4);
    }
    std::vector<float> offf(32);
    for (int m = 0; m < 32; ++m) { const int32_t v = best[m]; memcpy(&offf[m], &v, 4); }
    o.meloff = hb.add(offf.data(), 32);
    o.meldst = hb.add(dst.data(), 128);
    return 0;
}

// the 20 layers of the embedding CNN in the operand order of the handle's kernel family, each followed by its BatchNorm arrays
inline int pack_cnn(const PackIn& in, HostBuf& hb, WeightOff& o) {
    const float* q = in.emb_blob.data();
    std::vector<float> pk;
    for (int l = 0; l < 20; ++l) {
        const LayerDef& L = kLayers[l];
        const size_t nw = (size_t)L.kh * L.kw * L.cin * L.cout;
        const float* bn_scale = l < 19 ? q + nw : nullptr;             // folded inference BatchNorm of this layer (blob order: w, scale, shift)
        if (!in.mfma) o.conv[l] = hb.add(q, nw);
        else if (in.hx) {
            // fold_cnn: W' = s w 2^(e_out - e_in) per output channel (calibrate_hx's scale ladder; e_in = 0 for the mel input)
            std::vector<double> colmul(L.cout);
            const int de = in.hx_e[l] - in.hx_ein[l];
            for (int c = 0; c < L.cout; ++c) colmul[c] = std::ldexp(bn_scale ? (double)bn_scale[c] : 1.0, de);
            HxFold fold; fold.colmul = colmul.data();
            const bool time_merged = OWH_KMERGE && L.kh == 3 && L.kw == 1 && ((L.cin + 15) / 16) % 2 == 1 &&
                                     (L.cin % 16 == 8 || OWH_KMERGE_B);                     // stage C (and B): layers b, d
            // 1x3 layers with a 72-channel input (stage C layer c, stage D layer a): owh::conv_mel_hxm, same packing rule
            const bool mel_merged = OWH_KMERGE_MEL && owh::kInterleave && L.kh == 1 && L.kw == 3 &&
                                    ((L.cin + 15) / 16) % 2 == 1 && (L.cin + 15) / 16 >= 3 &&
                                    (L.cin % 16 == 8 || (OWH_KMERGE_MEL2 && l == 7 && OWH_WPS_C == 2) ||   // (l == 7: stage C layer a, 48 -> 72)
                                     (OWH_KMERGE_MEL2B && l == 5));                                   // (l == 5: stage B layer c, A/B switch)
            if (l == 0) pack_hx_conv0(q, pk, &fold);
            else if (l <= 2) pack_hx_stage_a(q, l, pk, &fold);
            else if (time_merged || mel_merged) pack_hx_tm(q, L.cin, L.cout, pk, &fold);
            else pack_hx(q, 3, L.cin, L.cout, pk, &fold, OWH_REM2 && !OWH_KMERGE_B && !OWH_KMERGE_MEL2B && l >= 4 && l <= 6);     // (stage B layers b, c, d)
            if (!(fold.absmax < 65000.0))
                return fail(OWW_ERANGE, "conv layer %d: folded weight magnitude %.3g (BatchNorm scale x weight x activation-scale ratio 2^%d) is outside "
                            "the f16 range of the fp16-split kernels (use_mfma = 3); use use_mfma = 1", l, fold.absmax, de);
            o.conv[l] = hb.add(pk);
        }
        else if (in.rr && l > 0) { pack_rr(q, 3, L.cin, L.cout, pk); o.conv[l] = hb.add(pk); }
        else if (l == 0) {
            // conv0: K = 9 taps padded to 12 -> three k-steps; lane (i, j) of k-step s holds w[k = 4s+j][cout = 16ct+i]
            pk.assign(2 * 3 * 64, 0.f);
            for (int ct = 0; ct < 2; ++ct)
                for (int s = 0; s < 3; ++s)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int k = 4 * s + (lane >> 4), co = ct * 16 + (lane & 15);
                        if (k < 9 && co < 24) pk[(ct * 3 + s) * 64 + lane] = q[k * 24 + co];
                    }
            o.conv[l] = hb.add(pk);
        } else { pack_mfma(q, 3, L.cin, L.cout, pk); o.conv[l] = hb.add(pk); }
        q += nw;
        if (l < 19) {
            // zero padded to whole 16-channel tiles: the register-resident kernels evaluate the pad channels (as zeros)
            std::vector<float> pad((size_t)(L.cout + 15) / 16 * 16, 0.f);
            if (in.hx) {
                // f16-split family: the scale lives in the weights.  Slot "scale" is only read by conv0: the third operand of the
                // med3 that applies its ReLU in the folded form (+inf where the BatchNorm scale is >= 0, -inf where it is negative)
                std::vector<float> bound(L.cout);
                for (int c = 0; c < L.cout; ++c) bound[c] = q[c] < 0.f ? -INFINITY : INFINITY;
                pad_hx_rows(bound.data(), L.cout, 1.0f, pad);
            }
            else memcpy(pad.data(), q, L.cout * sizeof(float));
            o.scale[l] = hb.add(pad); q += L.cout;
            std::fill(pad.begin(), pad.end(), 0.f);
            if (in.hx) pad_hx_rows(q, L.cout, std::ldexp(1.0f, in.hx_e[l]), pad);       // accumulator start values K h, tile row order
            else memcpy(pad.data(), q, L.cout * sizeof(float));
            o.shift[l] = hb.add(pad); q += L.cout;
        }
    }
    return 0;
}

// heads, first half: the natural arrays of every net (+ packed w2 for hidden == 64)
inline void pack_net_arrays(const PackIn& in, HostBuf& hb, WeightOff& off) {
    off.net.assign(in.nets.size(), WeightOff::Net{});
    for (size_t ni = 0; ni < in.nets.size(); ++ni) {
        const NetHost& n = in.nets[ni];
        WeightOff::Net& o = off.net[ni];
        if (n.rnn) { o.rnn = hb.add(n.rnn, n.rnn_floats); continue; }
        const size_t in = (size_t)n.T * 96, H = n.hidden, O = n.n_out;
        o.w1 = hb.add(n.w1, in * H); o.b1 = hb.add(n.b1, H);
        o.ln1g = n.has_ln ? hb.add(n.ln1g, H) : 0; o.ln1b = n.has_ln ? hb.add(n.ln1b, H) : 0;
        const size_t blk = H * H + H + (n.has_ln ? 2 * H : 0);
        o.blocks = n.n_blocks > 0 ? hb.add(n.blocks, (size_t)n.n_blocks * blk) : 0;      // (the generic kernel walks them in place)
        if (n.n_blocks > 0) {
            o.w2 = hb.add(n.w2, H * H); o.b2 = hb.add(n.b2, H);
            o.ln2g = n.has_ln ? hb.add(n.ln2g, H) : 0; o.ln2b = n.has_ln ? hb.add(n.ln2b, H) : 0;
        }
        o.w3 = hb.add(n.w3, H * O); o.b3 = hb.add(n.b3, O);
        if (n.hidden == 64 && n.n_blocks == 1) { std::vector<float> pk; pack_mfma(n.w2, 1, 64, 64, pk); o.w2pk = hb.add(pk); }
    }
}

// Where the heads' nets run: fast groups (MFMA head kernels), the generic kernel, the recurrent kernel
struct HeadGroups {
    std::vector<HeadGroup> groups;
    std::vector<int> generic_nets;    // indices into nets (with verifier right after its primary)
    std::vector<int> rnn_nets;        // recurrent heads (train.py:85-98): owk::heads_rnn_kernel, one launch per head
};

// heads, second half: the nets sorted into fast groups, generic nets and recurrent nets, and the image of every fast group
inline int pack_head_groups(const PackIn& in, HeadGroups& hg, HostBuf& hb, WeightOff& off) {
    // grouping: heads whose nets are all (hidden 64, n_out 1, sigmoid) share a fast group per T (<= 8 nets each)
    hg = HeadGroups{};
    for (size_t hi = 0; hi < in.heads.size(); ++hi) {
        const auto [nb, ne] = in.head_nets[hi];
        if (in.nets[nb].rnn) { hg.rnn_nets.push_back(nb); continue; }       // recurrent heads have their own kernel in every family
        bool fast = in.mfma;
        // the MFMA head kernels: sigmoid nets of one output and one hidden block; exactly 64 hidden units in the fp32 family
        // (heads64_kernel), up to 64 in the fp16-split family (zero-padded, see pack_hx_net)
        for (int ni = nb; ni < ne; ++ni)
            fast = fast && (in.nets[ni].hidden == 64 || (in.hx && in.nets[ni].hidden <= 64)) && in.nets[ni].n_out == 1 &&
                   in.nets[ni].final_act == 0 && in.nets[ni].n_blocks == 1;
        // the wide form of the fp16-split heads kernel: ungated nets of up to 128 hidden units and 8 outputs with one hidden block
        // (the released multiclass `timer`: docs/models/timers.md:9-27; train.py's default layer_dim = 128)
        bool wide = !fast && in.hx && in.mfma && ne - nb == 1 && !in.no_wide_heads;
        for (int ni = nb; ni < ne; ++ni) wide = wide && in.nets[ni].hidden <= 128 && in.nets[ni].n_out <= 8 && in.nets[ni].n_blocks == 1 && in.nets[ni].role == 0;
        if (!fast && !wide) { for (int ni = nb; ni < ne; ++ni) hg.generic_nets.push_back(ni); continue; }
        HeadGroup* g = nullptr;
        const int ht = wide ? 8 : 4;
        const int cap = in.hx ? 16 / ht : owk::HD_MAXNETS;                // heads_hx_kernel: at most sixteen hidden tiles per launch
        for (auto& gg : hg.groups) if (gg.T == in.nets[nb].T && gg.ht == ht && gg.n_nets + (ne - nb) <= cap) { g = &gg; break; }
        if (!g) { hg.groups.push_back(HeadGroup{}); g = &hg.groups.back(); g->T = in.nets[nb].T; g->n_nets = 0; g->ht = ht; }
        for (int ni = nb; ni < ne; ++ni) { g->nets.push_back(ni); g->n_nets++; }
    }
    // group images: the first layers of a group's nets side by side, HP = 16 ht columns per net -- for heads64_kernel (narrow groups,
    // with the concatenated b1) and, fp16-split family, for heads_hx_kernel -- then every net's pack_hx_net pieces
    for (auto& g : hg.groups) {
        const int HP = 16 * g.ht;
        g.NH = HP * g.n_nets;
        const size_t K = (size_t)g.T * 96;
        std::vector<float> wcat(K * g.NH, 0.f), pk;
        std::vector<double> colmul(g.NH);
        WeightOff::Group go;
        go.net.resize(g.n_nets);
        for (int gi = 0; gi < g.n_nets; ++gi) {
            const NetHost& n = in.nets[g.nets[gi]];
            if (in.hx && !hx_net_scales(n, g.ht, go.net[gi], in.probe_emb, in.probe_nb)) return fail(OWW_EINVAL, "head weights are not finite");
            place_w1(n, HP * gi, HP, g.NH, go.net[gi].e1, wcat, colmul);
        }
        if (g.ht == 4) {
            std::vector<float> bcat(g.NH, 0.f);
            for (int gi = 0; gi < g.n_nets; ++gi) memcpy(&bcat[64 * gi], in.nets[g.nets[gi]].b1, in.nets[g.nets[gi]].hidden * sizeof(float));
            pack_mfma(wcat.data(), g.T, 96, g.NH, pk);
            go.w1pk = hb.add(pk); go.b1cat = hb.add(bcat);
        }
        if (in.hx) {
            pack_hx_w1(wcat.data(), (int)K, g.NH, colmul.data(), pk);
            go.w1hx = hb.add(pk);
            for (int gi = 0; gi < g.n_nets; ++gi) pack_hx_net(in.nets[g.nets[gi]], g.ht, false, hb, go.net[gi]);
        }
        off.group.push_back(go);
    }
    return 0;
}

// voice-activity stand-in (always fp16-split MFMA kernels, whatever the CNN family)
inline int pack_vad(const PackIn& in, HostBuf& hb, WeightOff& o, float& gain, float& bd) {
    if (in.vad_blob.empty()) return 0;
    const float* q = in.vad_blob.data();
    gain = *q++;
    o.vhann = hb.add(q, 256); q += 256;
    std::vector<float> encw, encb(4 * 64, 0.f), pk;
    for (int l = 0; l < 4; ++l) {
        const int cin = kVadEnc[l][0], cout = kVadEnc[l][1];
        if (!hx_in_range(q, (size_t)3 * cin * cout)) return fail(OWW_EINVAL, "VAD encoder weights too large for the fp16-split kernels");
        pack_hx(q, 3, cin, cout, pk);
        encw.insert(encw.end(), pk.begin(), pk.end());
        q += (size_t)3 * cin * cout;
        memcpy(&encb[l * 64], q, cout * sizeof(float)); q += cout;
    }
    if (encw.size() != (size_t)owv::V_WFLOATS) return fail(OWW_EINVAL, "internal: VAD encoder image is %zu floats, expected %d", encw.size(), owv::V_WFLOATS);
    o.vencw = hb.add(encw); o.vencb = hb.add(encb);
    std::vector<float> lw, lb;
    for (int l = 0; l < 2; ++l) {
        if (!hx_in_range(q, (size_t)128 * 256)) return fail(OWW_EINVAL, "VAD LSTM weights too large for the fp16-split kernels");
        // columns regrouped so that the four gates of hidden tile u are neighbours: column 16 (4u + gate) + i <- gate * 64 + 16u + i
        std::vector<float> perm((size_t)128 * 256);
        for (int k = 0; k < 128; ++k)
            for (int u = 0; u < 4; ++u)
                for (int gt = 0; gt < 4; ++gt)
                    for (int i = 0; i < 16; ++i) perm[(size_t)k * 256 + 16 * (4 * u + gt) + i] = q[(size_t)k * 256 + gt * 64 + 16 * u + i];
        pack_hx(perm.data(), 1, 128, 256, pk);
        lw.insert(lw.end(), pk.begin(), pk.end());
        q += (size_t)128 * 256;
        lb.insert(lb.end(), q, q + 256); q += 256;
    }
    o.vlw = hb.add(lw); o.vlb = hb.add(lb);
    o.vwd = hb.add(q, 64); q += 64;
    bd = *q;
    return 0;
}

inline uint64_t fp_mix(uint64_t hsh, const void* data, size_t nbytes) {           // FNV-1a, 64 bit
    const unsigned char* b = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < nbytes; ++i) { hsh ^= b[i]; hsh *= 1099511628211ull; }
    return hsh;
}

}  // namespace owp
