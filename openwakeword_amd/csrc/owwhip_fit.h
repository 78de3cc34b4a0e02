// owwhip_fit.h -- fitting custom verifiers on the device (include/owwhip.h: oww_verifier_fit; custom_verifier_model.py:95-113:
// StandardScaler -> LogisticRegression), many problems per call, each solved in its dual.  Four kernels per slab of
// whole problems (owf::slab_plan), every one of them a function of its own problem's windows alone, in a fixed order of operations:
// a problem's (w, bias) does not depend on what else is in the call.
//  * fit_stats_kernel: one thread per (problem, column): mean and variance (ddof 0) of the column in fp64, s = 1 where the column is
//    exactly constant; z = (x - mu) / s rounded to fp32 and written once as f16 hi / lo halves (|z| <= sqrt(N - 1) <= 32: the f16
//    range holds by construction), row-major [row][D], so that a lane's 8 consecutive k of a row are one 16-byte load.  A column whose
//    sum is not finite raises the problem's flag.
//  * fit_gram_kernel: K = Z Z^T on v_mfma_f32_16x16x32_f16, hh + hl + lh with fp32 accumulation.  One wave per 32 x 32 tile on or
//    above the diagonal (owf::tile_map), 2 x 2 MFMA tiles; A and B operands are both rows of Z, loaded straight from global memory
//    (lane l: row l & 15, k = 8 (l >> 4) ..).  k runs 0 .. D in steps of 32 in one wave: a fixed order.  Rows behind the problem's
//    end read as zeros and are not stored; a tile off the diagonal is stored twice (mirrored), a diagonal tile stores its elements on
//    or above the diagonal and their mirrors, so the stored matrix is exactly symmetric.
//  * fit_solve_kernel: one workgroup of 1024 threads per problem: the Newton iteration on J(a, b) = C sum l(f_i) + 1/2 a^T K a,
//    f = K a + b, in fp32.  With p = sigmoid(f), g = p - y, W = p (1 - p), S = sqrt(W) and v = S (K da + db) a Newton step is
//        (I + C S K S) v = S (-K (C g + a) + db 1),    a + da = -C (g + S v),    sum_i (g_i + S_i v_i) = 0,
//    a symmetric positive definite system whatever K (duplicate windows) and W are.  v = v1 + db v2: two conjugate-gradient solves that
//    share every pass over K (read from global memory: L2-resident at these sizes; K is symmetric, so thread i walks column i and the
//    wave reads rows).  Thread t owns row t % NP of part t / NP of the k range (NP = N rounded up to a power of two, >= 64), and the
//    parts are summed in part order: every reduction has a fixed order.  Stop at res = max |a + C (p - y)| / C <= owf::kEpsStop or at
//    owf::kNewtonCap steps (not converged).  Step halving compares J only beyond its fp32 noise (owf::kJNoise).
//  * fit_fold_kernel: one workgroup per converged problem: w_j = (sum_i a_i z_ij) / s_j with z recomputed from the fp32 windows (fp64
//    accumulation), bias = b - sum_j w_j mu_j in fp64 (the cancellation DESIGN.md 8 warns about), both stored as fp32 straight into
//    the pool slot.
#pragma once
#include "owwhip_fit_host.h"
#include "owwhip_hx.h"

namespace owfk {

using owf::Problem;
using owf::Record;
using owf::Tile;
using owh::f16x8;
using owr::f32x4;

struct FitParams {
    const Problem* prob;
    const float* x;              // the slab's window base
    const unsigned char* y;      // the slab's labels
    _Float16* zh;                // [rows][D]
    _Float16* zl;
    double* mu;                  // [problems][D]
    double* sd;                  // [problems][D]
    float* K;                    // the slab's Gram matrices, compact [N][N] each
    float* a;                    // [rows]: the dual solution
    float* b;                    // [problems]
    int* flag;                   // [problems]: non-finite input
    Record* rec;                 // [problems]
    const Tile* tiles;
    int n_tiles, n_prob, D;
    float C;
    float* pool_w;
    float* pool_b;
    long long pool_stride;
};

// ---- statistics and operand staging: grid (ceil(D / 256), problems) ----
__global__ __launch_bounds__(256) void fit_stats_kernel(FitParams p) {
    const Problem pr = p.prob[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= p.D) return;
    const float* x = p.x + pr.x_off + j;
    const size_t D = (size_t)p.D;
    double sum = 0.0;
    for (int i = 0; i < pr.N; ++i) sum += (double)x[i * D];
    const double mu = sum / pr.N;
    double ss = 0.0;
    for (int i = 0; i < pr.N; ++i) { const double d = (double)x[i * D] - mu; ss += d * d; }
    const double var = ss / pr.N;
    const double sd = var == 0.0 ? 1.0 : sqrt(var);            // StandardScaler: an exactly constant column keeps its values' scale
    if (!(fabs(sum) <= 1.7e308) || !(ss <= 1.7e308)) p.flag[blockIdx.y] = 1;      // a NaN or an infinity in the column
    p.mu[(size_t)blockIdx.y * D + j] = mu;
    p.sd[(size_t)blockIdx.y * D + j] = sd;
    _Float16* zh = p.zh + (size_t)pr.z_row * D + j;
    _Float16* zl = p.zl + (size_t)pr.z_row * D + j;
    for (int i = 0; i < pr.N; ++i) {
        const float z = (float)(((double)x[i * D] - mu) / sd);
        const _Float16 h = (_Float16)z;
        zh[i * D] = h;
        zl[i * D] = (_Float16)(z - (float)h);
    }
}

// ---- batched Gram matrix: one wave per tile of owf::tile_map, 4 waves per workgroup ----
__global__ __launch_bounds__(256) void fit_gram_kernel(FitParams p) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= p.n_tiles) return;
    const Tile tl = p.tiles[t];
    const Problem pr = p.prob[tl.p];
    const int lane = threadIdx.x & 63, r16 = lane & 15, j = lane >> 4;
    const size_t D = (size_t)p.D;
    const int N = pr.N;
    // operand rows of this lane: row block q of the tile row (A) and of the tile column (B); behind the problem's end: zeros
    int rowA[2], rowB[2];
    const _Float16 *ah[2], *al[2], *bh[2], *bl[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        rowA[q] = tl.tr * owf::kTile + 16 * q + r16;
        rowB[q] = tl.tc * owf::kTile + 16 * q + r16;
        const size_t oa = ((size_t)pr.z_row + min(rowA[q], N - 1)) * D + 8 * j, ob = ((size_t)pr.z_row + min(rowB[q], N - 1)) * D + 8 * j;
        ah[q] = p.zh + oa; al[q] = p.zl + oa;
        bh[q] = p.zh + ob; bl[q] = p.zl + ob;
    }
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 acc[2][2];
#pragma unroll
    for (int qa = 0; qa < 2; ++qa)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) acc[qa][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < p.D; k += 32) {
        f16x8 Ah[2], Al[2], Bh[2], Bl[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const bool ina = rowA[q] < N, inb = rowB[q] < N;
            Ah[q] = ina ? *reinterpret_cast<const f16x8*>(ah[q] + k) : zero;
            Al[q] = ina ? *reinterpret_cast<const f16x8*>(al[q] + k) : zero;
            Bh[q] = inb ? *reinterpret_cast<const f16x8*>(bh[q] + k) : zero;
            Bl[q] = inb ? *reinterpret_cast<const f16x8*>(bl[q] + k) : zero;
        }
#pragma unroll
        for (int qa = 0; qa < 2; ++qa)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                acc[qa][qb] = OWH_MFMA(Ah[qa], Bh[qb], acc[qa][qb]);
                acc[qa][qb] = OWH_MFMA(Ah[qa], Bl[qb], acc[qa][qb]);
                acc[qa][qb] = OWH_MFMA(Al[qa], Bh[qb], acc[qa][qb]);
            }
    }
    // D[row 4 j + e][col r16] of MFMA tile (qa, qb)
    float* K = p.K + pr.k_off;
    const bool diag = tl.tr == tl.tc;
#pragma unroll
    for (int qa = 0; qa < 2; ++qa)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = tl.tr * owf::kTile + 16 * qa + 4 * j + e, c = tl.tc * owf::kTile + 16 * qb + r16;
                if (r >= N || c >= N || (diag && c < r)) continue;
                K[(size_t)r * N + c] = acc[qa][qb][e];
                if (c != r) K[(size_t)c * N + r] = acc[qa][qb][e];
            }
}

// ---- the solver ----
constexpr int kSolveThreads = 1024;

// sum of one value per thread, in a fixed order (tree over the 1024 slots); every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kSolveThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ float block_max(float v, double* red) {
    __syncthreads();
    red[threadIdx.x] = (double)v;
    __syncthreads();
    for (int s = kSolveThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return (float)red[0];
}

struct SolveLds {
    float t0[owf::kMaxN], t1[owf::kMaxN];          // the vectors a pass over K multiplies
    float part0[kSolveThreads], part1[kSolveThreads];
    double red[kSolveThreads];
};

// (o0, o1)[i] = sum_k K[k][i] (t0, t1)[k] for row i = threadIdx.x % NP, valid in the threads of part 0 (threadIdx.x < NP); K is
// symmetric, so column i is row i.  Part q of the k range is summed in k order, the parts in part order.
template <bool TWO>
__device__ __forceinline__ void k_pass(const float* K, int N, int NP, int per, SolveLds& L, float& o0, float& o1) {
    const int i = threadIdx.x & (NP - 1), part = threadIdx.x / NP;
    __syncthreads();                                // t0 / t1 written
    float s0 = 0.f, s1 = 0.f;
    if (i < N) {
        const int k1 = min(N, (part + 1) * per);
        for (int k = part * per; k < k1; ++k) {
            const float kv = K[(size_t)k * N + i];
            s0 = fmaf(kv, L.t0[k], s0);
            if (TWO) s1 = fmaf(kv, L.t1[k], s1);
        }
    }
    L.part0[threadIdx.x] = s0;
    if (TWO) L.part1[threadIdx.x] = s1;
    __syncthreads();
    o0 = 0.f; o1 = 0.f;
    if ((int)threadIdx.x < NP) {
        for (int q = 0; q < kSolveThreads / NP; ++q) {
            o0 += L.part0[q * NP + i];
            if (TWO) o1 += L.part1[q * NP + i];
        }
    }
    __syncthreads();                                // part0 / part1 and t0 / t1 free again
}

__device__ __forceinline__ float fit_sigmoid(float f) { return 1.f / (1.f + expf(-f)); }
__device__ __forceinline__ float fit_loss(float y, float f) { return fmaxf(f, 0.f) + log1pf(expf(-fabsf(f))) - y * f; }

__global__ __launch_bounds__(kSolveThreads) void fit_solve_kernel(FitParams p) {
    __shared__ SolveLds L;
    const Problem pr = p.prob[blockIdx.x];
    const int N = pr.N, tid = threadIdx.x;
    Record rec{OWW_FIT_NOT_CONVERGED, 0, 0.f, 0.f};
    if (p.flag[blockIdx.x]) {                       // (uniform: the whole workgroup leaves)
        if (tid == 0) { rec.status = OWW_FIT_NONFINITE; p.rec[blockIdx.x] = rec; }
        return;
    }
    int NP = 64;
    while (NP < N) NP <<= 1;
    const int parts = kSolveThreads / NP, per = (N + parts - 1) / parts;
    const float* K = p.K + pr.k_off;
    const float C = p.C;
    const bool own = tid < N;                       // thread i < N owns element i of every vector
    const float y = own ? (float)p.y[pr.y_off + tid] : 0.f;
    float a = 0.f, f = 0.f, b = 0.f;
    auto J_of = [&](float a_, float b_, float f_) {
        return (double)C * block_sum(own ? (double)fit_loss(y, f_) : 0.0, L.red) + 0.5 * block_sum(own ? (double)(a_ * (f_ - b_)) : 0.0, L.red);
    };
    double J = J_of(a, b, f);
    float res = 0.f;
    int it = 0;
    bool conv = false;
    const int cgcap = owf::cg_cap(N);
    while (it < owf::kNewtonCap) {
        ++it;
        const float pp = fit_sigmoid(f), g = own ? pp - y : 0.f, W = own ? pp * (1.f - pp) : 0.f, S = sqrtf(W);
        float kt, unused;
        if (own) L.t0[tid] = C * g + a;
        k_pass<false>(K, N, NP, per, L, kt, unused);
        // two systems (I + C S K S) x = rhs, rhs0 = -S kt, rhs1 = S
        float x0 = 0.f, x1 = 0.f, r0 = own ? -S * kt : 0.f, r1 = S, d0 = r0, d1 = r1;
        float rr0 = (float)block_sum((double)(r0 * r0), L.red), rr1 = (float)block_sum((double)(r1 * r1), L.red);
        const float tol0 = owf::kCgRtol2 * rr0, tol1 = owf::kCgRtol2 * rr1;
        for (int cg = 0; cg < cgcap; ++cg) {
            const bool live0 = rr0 > tol0, live1 = rr1 > tol1;
            if (!live0 && !live1) break;
            if (own) { L.t0[tid] = S * d0; L.t1[tid] = S * d1; }
            float k0, k1;
            k_pass<true>(K, N, NP, per, L, k0, k1);
            const float Ad0 = own ? d0 + C * S * k0 : 0.f, Ad1 = own ? d1 + C * S * k1 : 0.f;
            const float dAd0 = (float)block_sum((double)(d0 * Ad0), L.red), dAd1 = (float)block_sum((double)(d1 * Ad1), L.red);
            float rn0 = rr0, rn1 = rr1;
            if (live0) {
                if (dAd0 > 0.f) { const float al = rr0 / dAd0; x0 += al * d0; r0 -= al * Ad0; }
            }
            if (live1) {
                if (dAd1 > 0.f) { const float al = rr1 / dAd1; x1 += al * d1; r1 -= al * Ad1; }
            }
            rn0 = (float)block_sum((double)(r0 * r0), L.red);
            rn1 = (float)block_sum((double)(r1 * r1), L.red);
            if (live0) { if (dAd0 > 0.f) { d0 = r0 + (rn0 / rr0) * d0; rr0 = rn0; } else rr0 = 0.f; }
            if (live1) { if (dAd1 > 0.f) { d1 = r1 + (rn1 / rr1) * d1; rr1 = rn1; } else rr1 = 0.f; }
        }
        const float num = (float)block_sum(own ? (double)(g + S * x0) : 0.0, L.red), den = (float)block_sum((double)(S * x1), L.red);
        const float db = den > 0.f ? -num / den : 0.f;
        const float v = x0 + db * x1;
        const float an = own ? -C * (g + S * v) : 0.f, da = an - a;
        float ka;
        if (own) L.t0[tid] = an;
        k_pass<false>(K, N, NP, per, L, ka, unused);
        const float fn = own ? ka + (b + db) : 0.f, df = fn - f;
        float t = 1.f, a2 = an, b2 = b + db, f2 = fn;
        double J2 = J;
        for (int hv = 0; hv <= owf::kMaxHalvings; ++hv) {
            if (hv > 0) { a2 = a + t * da; b2 = b + t * db; f2 = f + t * df; }
            J2 = J_of(a2, b2, f2);
            if (J2 <= J + (double)owf::kJNoise * fabs(J) || hv == owf::kMaxHalvings) break;      // (uniform: J is the same in every thread)
            t *= 0.5f;
        }
        a = a2; b = b2; f = f2; J = J2;
        res = block_max(own ? fabsf(a + C * (fit_sigmoid(f) - y)) : 0.f, L.red) / C;
        if (res <= owf::kEpsStop) { conv = true; break; }
        if (!(res == res)) break;                   // NaN: nothing to iterate on
    }
    if (own) p.a[pr.z_row + tid] = a;
    if (tid == 0) {
        p.b[blockIdx.x] = b;
        rec.status = conv ? OWW_FIT_OK : OWW_FIT_NOT_CONVERGED;
        rec.iterations = it;
        rec.residual = res;
        p.rec[blockIdx.x] = rec;
    }
}

// ---- back-projection and fold: one workgroup per problem, straight into the pool slot ----
__global__ __launch_bounds__(256) void fit_fold_kernel(FitParams p) {
    __shared__ double red[256];
    __shared__ float a_s[owf::kMaxN];
    const Problem pr = p.prob[blockIdx.x];
    if (p.rec[blockIdx.x].status != OWW_FIT_OK) return;
    const size_t D = (size_t)p.D;
    for (int i = threadIdx.x; i < pr.N; i += 256) a_s[i] = p.a[pr.z_row + i];
    __syncthreads();
    float* w_out = p.pool_w + (size_t)pr.id * p.pool_stride;
    double acc_b = 0.0;
    for (int j = threadIdx.x; j < p.D; j += 256) {
        const double mu = p.mu[(size_t)blockIdx.x * D + j], sd = p.sd[(size_t)blockIdx.x * D + j];
        const float* x = p.x + pr.x_off + j;
        double s = 0.0;
        for (int i = 0; i < pr.N; ++i) s += (double)a_s[i] * (double)(float)(((double)x[i * D] - mu) / sd);
        const float w = (float)(s / sd);
        w_out[j] = w;
        acc_b += (double)w * mu;
    }
    red[threadIdx.x] = acc_b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.pool_b[pr.id] = (float)((double)p.b[blockIdx.x] - red[0]);
}

}  // namespace owfk
