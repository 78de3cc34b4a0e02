// owwhip_autotrain.h -- validating, checkpointing and merging the heads of a training session on the device (include/owwhip.h:
// oww_train_eval, oww_train_snapshot, oww_train_average; train.py:512-553, 557-567, 198-223).  Exact fp32 throughout.
//  * train_eval_kernel<NT>: train_fwd_kernel's forward half (owwhip_train.h) and nothing else, restated here statement for statement
//    so that the step's kernel keeps its own code: Z1 = X W1 on v_mfma_f32_16x16x4_f32 with the rows gathered by index and W1 staged
//    through LDS 32 input rows at a time, the rest of the network on four lanes per row, then the three comparisons of train.py:100
//    and of the binary Recall / Accuracy.  Grid (problems, tiles of 64 slots), problems fastest: with a shared table the workgroups
//    that are dispatched together read the same 64 pool rows, which the first of them brings into L2 for the others.  A workgroup
//    reads its own problem alone; the five counts are integers, summed in LDS and added to the problem's record with integer
//    atomics, so neither a score nor a count depends on what else is in the call or on how a table is cut.
//  * train_snapshot_kernel / train_average_kernel: 16-byte accesses over [U][stride], one thread per four parameters, no LDS and no
//    waiting across workgroups.  The average reads an element from every selected slot before it writes it, so the destination may
//    be one of them.
#pragma once
#include "owwhip_autotrain_host.h"
#include "owwhip_train.h"

namespace owak {

using owr::f32x4;
using owtk::kKC;
using owtk::quad_sum;

struct EvalParams {
    const float* par;                      // [U][stride]: the live parameters or one checkpoint slot
    const float* pool;                     // [P][F]: the eval pool
    const int* idx;                        // [rows][n]
    const unsigned char* y;
    float* scores;                         // [U][n] or null
    int* counts;                           // [U][5], zeroed before the launch
    long long tab_stride;                  // entries from one problem's table to the next (0: one table shared by all)
    long long stride;
    int P, F, n;
};

__host__ __device__ constexpr int eval_lds_floats(int NT) { return owt::kTileRows * (16 * NT + 1) + kKC * (16 * NT + 4) + 8; }

template <int NT>
__global__ __launch_bounds__(256) void train_eval_kernel(EvalParams p) {
    constexpr int D = 16 * NT, DS = D + 1, WS = D + 4, Q = 4 * NT, R = owt::kTileRows;
    extern __shared__ __attribute__((aligned(16))) float el[];
    float* bufA = el;                      // [R][DS]: Z1, then H1
    float* w1s = el + R * DS;              // [kKC][WS]: the W1 stage
    int* cnt_s = reinterpret_cast<int*>(el + R * DS + kKC * WS);
    const int u = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x;
    const float* par = p.par + (size_t)u * p.stride;
    const size_t tab = (size_t)u * p.tab_stride;
    const int F = p.F;
    if (tid < owa::kCounts) cnt_s[tid] = 0;

    // ---- Z1 = X W1 (train_fwd_kernel's, with the eval pool and the eval tables) ----
    {
        const int w = tid >> 6, lane = tid & 63, pp = lane & 15, j = lane >> 4;
        const int br = tile * R + 16 * w + pp;
        int ix = br < p.n ? p.idx[tab + br] : -1;
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
#pragma unroll
        for (int dt = 0; dt < NT; ++dt)
#pragma unroll
            for (int e = 0; e < 4; ++e) bufA[(16 * w + pp) * DS + 16 * dt + 4 * j + e] = acc[dt][e];
    }
    __syncthreads();

    // ---- the rest of the network: four lanes per row ----
    const int r = tid >> 2, q = tid & 3, d0 = q * Q;
    const int br = tile * R + r;
    const int ix = br < p.n ? p.idx[tab + br] : -1;
    const bool valid = ix >= 0 && ix < p.P;
    const int yv = br < p.n ? (int)p.y[tab + br] : 0;
    const float *b1 = par + (size_t)F * D, *g1 = b1 + D, *be1 = g1 + D, *W2 = be1 + D, *b2 = W2 + D * D, *g2 = b2 + D, *be2 = g2 + D,
                *w3 = be2 + D, *b3 = w3 + D;
    constexpr float invD = 1.f / D;
    {
        float z[Q], s = 0.f;
#pragma unroll
        for (int c = 0; c < Q; ++c) { z[c] = bufA[r * DS + d0 + c] + b1[d0 + c]; s += z[c]; }
        const float mu = quad_sum(s) * invD;
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < Q; ++c) { z[c] -= mu; ss += z[c] * z[c]; }
        const float rstd1 = 1.f / sqrtf(quad_sum(ss) * invD + 1e-5f);
#pragma unroll
        for (int c = 0; c < Q; ++c) {
            const float xh = z[c] * rstd1;
            const float a = xh * g1[d0 + c] + be1[d0 + c];
            bufA[r * DS + d0 + c] = fmaxf(a, 0.f);
        }
    }
    __syncthreads();
    float h2[Q];
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
        const float rstd2 = 1.f / sqrtf(quad_sum(ss) * invD + 1e-5f);
#pragma unroll
        for (int c = 0; c < Q; ++c) {
            const float xh = z[c] * rstd2;
            const float a = xh * g2[d0 + c] + be2[d0 + c];
            h2[c] = fmaxf(a, 0.f);
        }
    }
    float lg = 0.f;
#pragma unroll
    for (int c = 0; c < Q; ++c) lg = fmaf(h2[c], w3[d0 + c], lg);
    lg = quad_sum(lg) + b3[0];
    const float pr = 1.f / (1.f + expf(-lg));

    // ---- the comparisons: train.py:100 (y - p <= -0.5: y = 0 and p >= 0.5) and the binary Recall / Accuracy rule (p > 0.5) ----
    if (q == 0 && br < p.n) {
        if (p.scores) p.scores[(size_t)u * p.n + br] = valid ? pr : __builtin_nanf("");
        if (valid) {
            atomicAdd(&cnt_s[yv ? 0 : 1], 1);
            if (pr > 0.5f) atomicAdd(&cnt_s[yv ? 2 : 3], 1);
            if (!yv && pr >= 0.5f) atomicAdd(&cnt_s[4], 1);
        }
    }
    __syncthreads();
    if (tid < owa::kCounts && cnt_s[tid]) atomicAdd(&p.counts[(size_t)u * owa::kCounts + tid], cnt_s[tid]);
}

// problem u's live record -> its slot slot[u] (-1: none).  grid (groups of 1024 floats, problems)
__global__ __launch_bounds__(256) void train_snapshot_kernel(const float* par, float* ckpt, const int* slot, long long stride, int U) {
    const int u = blockIdx.y, s = slot[u];
    const long long e = 4ll * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (s < 0 || e >= stride) return;
    const f32x4 v = *reinterpret_cast<const f32x4*>(par + (size_t)u * stride + e);
    *reinterpret_cast<f32x4*>(ckpt + ((size_t)s * U + u) * stride + e) = v;
}

// average_models (train.py:198-223) per problem over the slots sel [U][C] marks, into slot dst; none marked: the live record
__global__ __launch_bounds__(256) void train_average_kernel(const float* par, float* ckpt, const unsigned char* sel, long long stride, int U,
                                                            int C, int dst) {
    const int u = blockIdx.y;
    const long long e = 4ll * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (e >= stride) return;
    const unsigned char* su = sel + (size_t)u * C;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int c = 0; c < C; ++c) {
        if (!su[c]) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(ckpt + ((size_t)c * U + u) * stride + e);
        if (cnt == 0) {                    // the deep copy of models[0], "*= 0"
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = v[i] * 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += v[i];
        ++cnt;
    }
    if (cnt == 0) {
        acc = *reinterpret_cast<const f32x4*>(par + (size_t)u * stride + e);
    } else {
        const float fc = (float)cnt;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = acc[i] / fc;
    }
    *reinterpret_cast<f32x4*>(ckpt + ((size_t)dst * U + u) * stride + e) = acc;
}

}  // namespace owak
