// owwhip_train.h -- training bank heads on the device (include/owwhip.h: oww_train_*; train.py:434-510 for the network of
// train.py:66-83 with n_blocks = 1, n_classes = 1), U independent problems side by side.  One step is three
// launches that each cover all problems; every workgroup reads its own problem alone and every reduction has a fixed order, so a
// problem's bits do not depend on what else is in the call.  Exact fp32 throughout (NT = hidden / 16).
//  * train_fwd_kernel<NT>: grid (tiles of 64 batch rows, problems), 4 waves.  Z1 = X W1 on v_mfma_f32_16x16x4_f32: wave w owns rows
//    16 w .. 16 w + 15, gathered from the pool by index (operand B: lane (p, j) loads X[row p][.. + 4 j .. 4 j + 3], one 16-byte
//    load = four k-steps; k-step e of it carries inputs {4 j + e}); W1 is staged through LDS 32 input rows at a time (operand A:
//    lane (i, j) reads W1[4 j + e][16 dt + i]).  The rest of the network runs on four lanes per row (lane q owns units q D/4 ..):
//    LayerNorm, ReLU, the D x D layer (W2 read from global memory, L1-resident), LayerNorm, ReLU, the output unit, the sigmoid, the
//    selection of train.py:464-465, the weighted BCE and its gradient at the logit as binary_cross_entropy and Sigmoid compute it in
//    fp32, then the backward pass down to dZ1.  It leaves the tile's dZ1 rows (zeros for dropped, empty and padding rows), kept
//    count, loss partial and the partial sums of every parameter but W1, each summed over the tile's rows in row order.  Nothing is
//    scaled by 1 / (m acc_steps) here: that factor is linear and applied downstream, so no workgroup waits for a whole-batch count.
//  * train_w1_kernel<NT>: grid (groups of 64 input columns, problems).  gW1 = X^T dZ1 on the same MFMA with the batch axis as the k
//    loop, rows 0 .. n_pad in one walk; a wave owns 16 inputs x all hidden units and lane (p, j) ends with the four consecutive
//    elements W1[f0 + p][16 dt + 4 j ..]: their Adam moments and weights are updated there as one 16-byte access each.
//  * train_small_kernel: one workgroup per problem: the tile partials of the other parameters are summed in tile order, Adam is
//    applied, the counters move and the step's record (loss, kept count) is written.
// The step / skip decision and the scale are recomputed by every workgroup of the last two kernels from the integer tile counts and
// the problem's counters, which only train_small_kernel writes, behind every reader of the step.
#pragma once
#include "owwhip_train_host.h"
#include "owwhip_rr.h"

namespace owtk {

using owr::f32x4;
using owt::Counters;
using owt::StepRecord;

struct TrainParams {
    float* par; float* am; float* av;      // [U][stride]: parameters and Adam's two moments
    Counters* cnt;                         // [U]
    const float* pool;                     // [P][F]
    const int* idx;                        // tables of the call: [rows][K][n_batch]
    const unsigned char* y;
    const double* lr;                      // [K]
    const float* nw;                       // [K]
    float* dz1;                            // [U][n_pad][D]
    float* part;                           // [U][n_tiles][small]
    int* tcount;                           // [U][n_tiles]
    float* tloss;                          // [U][n_tiles]
    StepRecord* rec;                       // [U][K]
    long long tab_stride;                  // entries from one problem's table to the next (0: one table shared by all)
    long long stride, small;
    int P, F, D, k, K, n_batch, n_tiles, n_pad;
};

constexpr int kKC = 32;                    // input rows of W1 staged per pass
__host__ __device__ constexpr int fwd_lds_floats(int NT) { return 2 * owt::kTileRows * (16 * NT + 1) + 3 * owt::kTileRows; }
static_assert(kKC * (128 + 4) <= owt::kTileRows * (128 + 1), "the W1 stage fits in the second row buffer");

__device__ __forceinline__ float quad_sum(float v) {       // over the 4 lanes of a row; the same bits in all four
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v;
}

// what every workgroup of a step derives from the tile counts and the counters: m, whether the optimizer steps, and the scale
struct Decision { int m; bool step; float scale; };
__device__ __forceinline__ Decision decide(const TrainParams& p, int u, const Counters& c) {
    int m = 0;
    for (int i = 0; i < p.n_tiles; ++i) m += p.tcount[(size_t)u * p.n_tiles + i];
    Decision d;
    d.m = m;
    d.step = m > 0 && c.acc_samples + m >= owt::kAccumulate;
    d.scale = m > 0 ? (1.f / (float)c.acc_steps) / (float)m : 0.f;
    return d;
}

// torch.optim.Adam's defaults (single-tensor path): the hyper-parameters of optimizer step t in double, applied in fp32
struct AdamStep { float step_size, bc2_sqrt; };
__device__ __forceinline__ AdamStep adam_step(double lr, int t) {
    AdamStep a;
    a.step_size = (float)(lr / (1.0 - pow(0.9, (double)t)));
    a.bc2_sqrt = (float)sqrt(1.0 - pow(0.999, (double)t));
    return a;
}
__device__ __forceinline__ void adam_update(float& w, float& m, float& v, float g, const AdamStep& a) {
    m = m + (g - m) * (float)(1.0 - 0.9);
    v = v * 0.999f + ((float)(1.0 - 0.999) * g) * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + 1e-8f;
    w = w + (-a.step_size * m) / denom;
}

template <int NT>
__global__ __launch_bounds__(256) void train_fwd_kernel(TrainParams p) {
    constexpr int D = 16 * NT, DS = D + 1, WS = D + 4, Q = 4 * NT, R = owt::kTileRows;
    extern __shared__ __attribute__((aligned(16))) float tl[];
    float* bufA = tl;                      // [R][DS]: Z1, then H1
    float* bufB = tl + R * DS;             // [R][DS]: the W1 stage, then dZ2, then column sums
    float* w1s = bufB;
    int* kept_s = reinterpret_cast<int*>(tl + 2 * R * DS);
    float* loss_s = tl + 2 * R * DS + R;
    float* g_s = tl + 2 * R * DS + 2 * R;
    const int tile = blockIdx.x, u = blockIdx.y, tid = threadIdx.x;
    const float* par = p.par + (size_t)u * p.stride;
    const size_t tab = (size_t)u * p.tab_stride + (size_t)p.k * p.n_batch;
    const int F = p.F;

    // ---- Z1 = X W1 ----
    {
        const int w = tid >> 6, lane = tid & 63, pp = lane & 15, j = lane >> 4;
        const int br = tile * R + 16 * w + pp;
        int ix = br < p.n_batch ? p.idx[tab + br] : -1;
        const bool valid = ix >= 0 && ix < p.P;
        const float* xrow = p.pool + (size_t)(valid ? ix : 0) * F + 4 * j;
        f32x4 acc[NT];
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int f0 = 0; f0 < F; f0 += kKC) {
            __syncthreads();
            const float* src = par + (size_t)f0 * D;
#pragma unroll
            for (int i = 0; i < 2 * NT; ++i) {
                const int e = tid + 256 * i;
                w1s[(e / D) * WS + (e % D)] = src[e];
            }
            __syncthreads();
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
                if (valid) x = *reinterpret_cast<const f32x4*>(xrow + f0 + 16 * hh);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int dt = 0; dt < NT; ++dt)
                        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1s[(16 * hh + 4 * j + e) * WS + 16 * dt + pp], x[e], acc[dt], 0, 0, 0);
            }
        }
        __syncthreads();                   // the stage is free: bufB is written from here on
#pragma unroll
        for (int dt = 0; dt < NT; ++dt)
#pragma unroll
            for (int e = 0; e < 4; ++e) bufA[(16 * w + pp) * DS + 16 * dt + 4 * j + e] = acc[dt][e];
    }
    __syncthreads();

    // ---- the rest of the network and its backward pass: four lanes per row ----
    const int r = tid >> 2, q = tid & 3, d0 = q * Q;
    const int br = tile * R + r;
    const int ix = br < p.n_batch ? p.idx[tab + br] : -1;
    const bool valid = ix >= 0 && ix < p.P;
    const int yv = br < p.n_batch ? (int)p.y[tab + br] : 0;
    const float *b1 = par + (size_t)F * D, *g1 = b1 + D, *be1 = g1 + D, *W2 = be1 + D, *b2 = W2 + D * D, *g2 = b2 + D, *be2 = g2 + D,
                *w3 = be2 + D, *b3 = w3 + D;
    constexpr float invD = 1.f / D;
    float xh1[Q], rstd1;
    unsigned pos1 = 0;
    {
        float z[Q], s = 0.f;
#pragma unroll
        for (int c = 0; c < Q; ++c) { z[c] = bufA[r * DS + d0 + c] + b1[d0 + c]; s += z[c]; }
        const float mu = quad_sum(s) * invD;
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < Q; ++c) { z[c] -= mu; ss += z[c] * z[c]; }
        rstd1 = 1.f / sqrtf(quad_sum(ss) * invD + 1e-5f);
#pragma unroll
        for (int c = 0; c < Q; ++c) {
            xh1[c] = z[c] * rstd1;
            const float a = xh1[c] * g1[d0 + c] + be1[d0 + c];
            if (a > 0.f) pos1 |= 1u << c;
            bufA[r * DS + d0 + c] = fmaxf(a, 0.f);
        }
    }
    __syncthreads();
    float xh2[Q], h2[Q], rstd2;
    unsigned pos2 = 0;
    {
        float z[Q];
#pragma unroll
        for (int c = 0; c < Q; ++c) z[c] = b2[d0 + c];
        for (int k = 0; k < D; ++k) {
            const float hk = bufA[r * DS + k];
#pragma unroll
            for (int c4 = 0; c4 < NT; ++c4) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(W2 + (size_t)k * D + d0 + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) z[4 * c4 + e] = fmaf(hk, wv[e], z[4 * c4 + e]);
            }
        }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < Q; ++c) s += z[c];
        const float mu = quad_sum(s) * invD;
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < Q; ++c) { z[c] -= mu; ss += z[c] * z[c]; }
        rstd2 = 1.f / sqrtf(quad_sum(ss) * invD + 1e-5f);
#pragma unroll
        for (int c = 0; c < Q; ++c) {
            xh2[c] = z[c] * rstd2;
            const float a = xh2[c] * g2[d0 + c] + be2[d0 + c];
            if (a > 0.f) pos2 |= 1u << c;
            h2[c] = fmaxf(a, 0.f);
        }
    }
    float lg = 0.f;
#pragma unroll
    for (int c = 0; c < Q; ++c) lg = fmaf(h2[c], w3[d0 + c], lg);
    lg = quad_sum(lg) + b3[0];
    const float pr = 1.f / (1.f + expf(-lg));
    const bool kept = valid && (yv ? pr < owt::kSelPos : pr >= owt::kSelNeg);
    const float wt = yv ? 1.f : p.nw[p.k];
    // F.binary_cross_entropy and Sigmoid, forward and backward, as ATen computes them in fp32
    const float bce = ((float)yv - 1.f) * fmaxf(log1pf(-pr), -100.f) - (float)yv * fmaxf(logf(pr), -100.f);
    const float sp = (1.f - pr) * pr;
    const float g = kept ? ((pr - (float)yv) / fmaxf(sp, 1e-12f)) * wt * sp : 0.f;
    if (q == 0) { kept_s[r] = kept ? 1 : 0; loss_s[r] = kept ? bce * wt : 0.f; g_s[r] = g; }

    // ---- backward ----
    float *part = p.part + ((size_t)u * p.n_tiles + tile) * p.small;
    const int o_b1 = 0, o_g1 = D, o_be1 = 2 * D, o_w2 = 3 * D, o_b2 = o_w2 + D * D, o_g2 = o_b2 + D, o_be2 = o_g2 + D, o_w3 = o_be2 + D, o_b3 = o_w3 + D;
    float da2[Q], dz2[Q];
    {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < Q; ++c) {
            da2[c] = (pos2 >> c & 1u) ? g * w3[d0 + c] : 0.f;
            dz2[c] = da2[c] * g2[d0 + c];                  // d xhat
            s1 += dz2[c];
            s2 = fmaf(dz2[c], xh2[c], s2);
        }
        const float m1 = quad_sum(s1) * invD, m2 = quad_sum(s2) * invD;
#pragma unroll
        for (int c = 0; c < Q; ++c) {
            dz2[c] = kept ? rstd2 * (dz2[c] - m1 - xh2[c] * m2) : 0.f;
            bufB[r * DS + d0 + c] = dz2[c];
        }
    }
    __syncthreads();                       // H1 in bufA, dZ2 in bufB
    {                                      // gW2[k][d] = sum over the tile's rows, in row order
        float acc[NT * NT];
#pragma unroll
        for (int i = 0; i < NT * NT; ++i) acc[i] = 0.f;
        for (int rr = 0; rr < R; ++rr)
#pragma unroll
            for (int i = 0; i < NT * NT; ++i) {
                const int o = tid + 256 * i;
                acc[i] = fmaf(bufA[rr * DS + o / D], bufB[rr * DS + o % D], acc[i]);
            }
#pragma unroll
        for (int i = 0; i < NT * NT; ++i) part[o_w2 + tid + 256 * i] = acc[i];
        if (tid < D) {                     // gb2
            float s = 0.f;
            for (int rr = 0; rr < R; ++rr) s += bufB[rr * DS + tid];
            part[o_b2 + tid] = s;
        }
    }
    float da1[Q], dz1[Q];
    {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < Q; ++c) {
            float s = 0.f;
            const float* wrow = W2 + (size_t)(d0 + c) * D;
            for (int dd = 0; dd < D; dd += 4) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wrow + dd);
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fmaf(bufB[r * DS + dd + e], wv[e], s);
            }
            da1[c] = (pos1 >> c & 1u) ? s : 0.f;
            dz1[c] = da1[c] * g1[d0 + c];
            s1 += dz1[c];
            s2 = fmaf(dz1[c], xh1[c], s2);
        }
        const float m1 = quad_sum(s1) * invD, m2 = quad_sum(s2) * invD;
        float* out = p.dz1 + ((size_t)u * p.n_pad + br) * D + d0;
#pragma unroll
        for (int c = 0; c < Q; ++c) {
            dz1[c] = kept ? rstd1 * (dz1[c] - m1 - xh1[c] * m2) : 0.f;
            out[c] = dz1[c];
        }
    }
    // column sums over the tile's rows, two vectors per round: threads 0 .. D - 1 sum bufA's columns, 128 .. 128 + D - 1 bufB's
    auto col_sums = [&](const float (&va)[Q], const float (&vb)[Q], int oa, int ob) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < Q; ++c) { bufA[r * DS + d0 + c] = va[c]; bufB[r * DS + d0 + c] = vb[c]; }
        __syncthreads();
        const int col = tid & 127;
        if (col < D) {
            const float* src = tid < 128 ? bufA : bufB;
            float s = 0.f;
            for (int rr = 0; rr < R; ++rr) s += src[rr * DS + col];
            part[(tid < 128 ? oa : ob) + col] = s;
        }
    };
    float t0[Q], t1[Q];
#pragma unroll
    for (int c = 0; c < Q; ++c) { t0[c] = da2[c] * xh2[c]; t1[c] = g * h2[c]; }
    col_sums(t0, da2, o_g2, o_be2);
    col_sums(t1, dz1, o_w3, o_b1);
#pragma unroll
    for (int c = 0; c < Q; ++c) t0[c] = da1[c] * xh1[c];
    col_sums(t0, da1, o_g1, o_be1);
    if (tid == 0) {
        int m = 0;
        float ls = 0.f, gs = 0.f;
        for (int rr = 0; rr < R; ++rr) { m += kept_s[rr]; ls += loss_s[rr]; gs += g_s[rr]; }
        p.tcount[(size_t)u * p.n_tiles + tile] = m;
        p.tloss[(size_t)u * p.n_tiles + tile] = ls;
        part[o_b3] = gs;
    }
}

template <int NT>
__global__ __launch_bounds__(256) void train_w1_kernel(TrainParams p) {
    constexpr int D = 16 * NT;
    const int u = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63, pp = lane & 15, j = lane >> 4;
    const int f0 = (blockIdx.x * 4 + w) * 16;
    if (f0 >= p.F) return;
    const Counters c = p.cnt[u];
    const Decision dec = decide(p, u, c);
    if (!dec.step) return;
    const size_t tab = (size_t)u * p.tab_stride + (size_t)p.k * p.n_batch;
    const float* dz = p.dz1 + (size_t)u * p.n_pad * D + pp;
    f32x4 acc[NT];
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.n_pad; k0 += 4) {
        const int row = k0 + j;
        const int ix = row < p.n_batch ? p.idx[tab + row] : -1;
        const float x = ix >= 0 && ix < p.P ? p.pool[(size_t)ix * p.F + f0 + pp] : 0.f;
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[(size_t)row * D + 16 * dt], x, acc[dt], 0, 0, 0);
    }
    // lane (p, j), register e of tile dt: gW1[f0 + p][16 dt + 4 j + e]
    const AdamStep a = adam_step(p.lr[p.k], c.opt_steps + 1);
    const size_t base = (size_t)u * p.stride + (size_t)(f0 + pp) * D + 4 * j;
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) {
        f32x4 wv = *reinterpret_cast<f32x4*>(p.par + base + 16 * dt), mv = *reinterpret_cast<f32x4*>(p.am + base + 16 * dt),
              vv = *reinterpret_cast<f32x4*>(p.av + base + 16 * dt);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float we = wv[e], me = mv[e], ve = vv[e];
            adam_update(we, me, ve, acc[dt][e] * dec.scale, a);
            wv[e] = we; mv[e] = me; vv[e] = ve;
        }
        *reinterpret_cast<f32x4*>(p.par + base + 16 * dt) = wv;
        *reinterpret_cast<f32x4*>(p.am + base + 16 * dt) = mv;
        *reinterpret_cast<f32x4*>(p.av + base + 16 * dt) = vv;
    }
}

__global__ __launch_bounds__(256) void train_small_kernel(TrainParams p) {
    const int u = blockIdx.x;
    const Counters c = p.cnt[u];
    const Decision dec = decide(p, u, c);
    if (dec.step) {
        const AdamStep a = adam_step(p.lr[p.k], c.opt_steps + 1);
        const float* part = p.part + (size_t)u * p.n_tiles * p.small;
        const size_t sb = (size_t)u * p.stride + (size_t)p.F * p.D;       // the record behind w1
        for (int e = threadIdx.x; e < p.small; e += 256) {
            float s = 0.f;
            for (int i = 0; i < p.n_tiles; ++i) s += part[(size_t)i * p.small + e];
            float we = p.par[sb + e], me = p.am[sb + e], ve = p.av[sb + e];
            adam_update(we, me, ve, s * dec.scale, a);
            p.par[sb + e] = we; p.am[sb + e] = me; p.av[sb + e] = ve;
        }
    }
    __syncthreads();                       // every thread has read the counters
    if (threadIdx.x == 0) {
        StepRecord rec{__builtin_nanf(""), dec.m};
        Counters n = c;
        if (dec.step) {
            float ls = 0.f;
            for (int i = 0; i < p.n_tiles; ++i) ls += p.tloss[(size_t)u * p.n_tiles + i];
            rec.loss = (ls / (float)dec.m) / (float)c.acc_steps;
            n.acc_steps = 1; n.acc_samples = 0; n.opt_steps = c.opt_steps + 1;
        } else if (dec.m > 0) {
            n.acc_steps = c.acc_steps + 1; n.acc_samples = c.acc_samples + dec.m;
        }
        p.cnt[u] = n;
        p.rec[(size_t)u * p.K + p.k] = rec;
    }
}

}  // namespace owtk
