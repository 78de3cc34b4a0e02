// owwhip_dense.h -- dense scoring (include/owwhip.h: oww_score_features, oww_score_clips): every T-row window of a feature sequence
// through the fp16-split heads.  Consecutive windows share T - 1 of their T rows, so a workgroup that scores a TILE of consecutive
// windows stages the tile's rows once -- scaled by fscale and split into f16 hi / lo by the very split_pair<false> the heads kernel
// uses -- and every k-step reads its B operand from LDS instead of loading and splitting its own rows: 1 / T of the feature traffic
// and of the splits of heads_hx_kernel on the materialised windows.
//
// heads_dense_kernel<NN, NBUF, WG>: one workgroup = WG waves x 2 position tiles of 16 = 32 WG consecutive windows of one sequence
// (WG = 8: 256 windows, or 4 where the rows of 256 do not fit), NN <= 2 narrow nets (HT = 4 hidden tiles) of one fast group -- a PASS
// (owd::split_passes) -- on the group's packed weights as they are (FastGroup::d_w1hx, hx_net): a pass reads its own nets' blocks of
// every k-step chunk.  At full size the heads launches are bound by the weight stream L2 -> LDS, once per workgroup; 256 windows per
// workgroup halve it against heads_hx_kernel's 128, which the compact rows in LDS make room for.
//  * staging (dense_stage_rows): rows [w0, w0 + 32 WG + T - 1) of the sequence (clamped to its last row: the windows that would read
//    beyond it are not stored) -> LDS, row stride owd::kRowWords = 100 words, unit (c, j) of a row = 8 hi halves | 8 lo halves
//    (owd::unit_word): the 16 positions of a tile, one row apart, read 16 distinct groups of 4 banks.
//  * k loop: k-step ks = (row tr = ks / 3, features 32 (ks % 3) ..) of every window; position pos of tile t of wave v reads staged row
//    32 v + 16 t + pos + tr.  The weight chunks stream L2 -> LDS through a ring of NBUF slots, each its OWN LDS object (hslot<>, see
//    heads_hx_kernel: one array would make every read of the current slot wait for the chunk just issued); dense_ring_prologue issues
//    the first NBUF - 1.  The same MFMAs in the same order as heads_hx_kernel -- per k-step and pair of hidden tiles (A hi, B hi),
//    (A hi, B lo), (A lo, B hi), tile 0 then tile 1 -- so an accumulator holds bit for bit what heads_hx_kernel's holds for the
//    materialised window.
//  * barrier discipline: heads_hx_kernel's wait for chunk ks + 1 rides on its feature loads (younger than the chunk, in-order return).
//    Here no VMEM load follows the chunks, so the wait is counted: every wave issues exactly 8 NN / WG DMA instructions per chunk
//    (issue_chunk_uniform), D = NBUF - 1 chunks fly ahead, and at the end of k-step ks "at most (D - 1) x 8 NN / WG outstanding" means this
//    wave's part of chunk ks + 1 has landed; the bare s_barrier (no release fence: it would be vmcnt(0)) publishes the other waves'
//    parts.  The slot refilled in k-step ks is the one k-step ks - 1 read: every wave passed that k-step's barrier with its LDS reads
//    returned (lgkmcnt(0)).  The last D k-steps wait vmcnt(0).  So the k loop must be entered with the first D chunks landed in every
//    wave and nothing else outstanding in vmcnt, and it ends without a barrier.
//  * tail: net64_score, the function form of heads_hx_kernel's narrow tail that the bank kernel already runs bit for bit, then the
//    gating of heads_hx_kernel.  No post-processing: dense scores are raw head outputs.
// heads_dense_bank_kernel<NBUF, WG> (further down) is the same over the head bank, with the head a loop variable.  The two kernels
// share the staging, the ring prologue and the statistics' commit step as functions.  The k loop stays INLINE in both, two copies of
// one text (the bank's reads staged row + t_s - T and strides its own CHUNK): as a shared function -- scalars by value or by
// reference, the stride an argument or a template policy, the staged rows, the lane's first row or the B-operand loader handed in by
// the caller, acc and the B operands caller-owned -- the fixed kernel's twelve instantiations keep their registers, but every form
// moved the bank kernel's register allocation: 19 to 28 SGPR spills where it has 18 / 26, and 40 to 160 instructions more per
// instantiation (outside the k loop: the statistics pointers no longer stay in SGPRs across it).  The same hazard as the note above
// heads_gemm1 (owwhip_hx.h) records for heads_hx_kernel; a change to one k loop is made in the other by hand, and
// tests/test_dense_bank_gpu.py holds the two to the same bits.
// A workgroup's LDS (108 KB of rows at T = 16 plus the ring) leaves no room for a second one on the CU, so the ring is as deep as fits
// (owd::geometry: 4, 3 or 2 slots) -- chunks in flight and the second wave of each SIMD, not neighbours, hide the L2 round trip.
//
// dense_gather_kernel: the fallback's window materialisation, [n][T][96] into a slab that owk / owh head kernels score as external
// features (run_heads ext) -- every head form the sliding kernel does not cover, bit-identical to oww_head by construction.
#pragma once
#include "owwhip_dense_bank_host.h"
#include "owwhip_dense_host.h"
#include "owwhip_hx.h"

namespace owh {

// ---- the pieces both sliding kernels are made of ------------------------------------------------------------------------------------
// Rows [w0, w0 + 32 WG + t_stage - 1) of `seq` (clamped to row n_rows - 1) -> dense_rows: scale, split, store in B-operand order, four
// units per thread in flight.  No barrier of its own: the caller publishes the rows.
template <int WG>
__device__ __forceinline__ void dense_stage_rows(float* dense_rows, const float* seq, const int w0, const int n_rows, const int t_stage, const float fsc) {
    using namespace owr;
    const int NU = (32 * WG + t_stage - 1) * 12;
    for (int u0 = threadIdx.x; u0 < NU; u0 += 4 * 64 * WG) {
        f32x4 r[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = min(u0 + q * 64 * WG, NU - 1);
            const int row = u / 12, unit = u - row * 12;
            const float* src = seq + (size_t)min(w0 + row, n_rows - 1) * 96 + unit * 8;
            r[q][0] = *reinterpret_cast<const f32x4*>(src);
            r[q][1] = *reinterpret_cast<const f32x4*>(src + 4);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = u0 + q * 64 * WG;
            if (u >= NU) continue;
            const int row = u / 12, unit = u - row * 12;
            const Op o = split_pair<false>(r[q][0] * fsc, r[q][1] * fsc);
            float* dst = dense_rows + owd::unit_word(row, unit);
            *reinterpret_cast<f16x8*>(dst) = o.h;
            *reinterpret_cast<f16x8*>(dst + 4) = o.l;
        }
    }
}

// The first D = NBUF - 1 k-step chunks of w1hx (NCT hidden tiles; chunk_stride floats apart) into ring slots 0 .. D-1.  (A net has
// 3 T >= 3 >= D k-steps: every prologue chunk exists.)
template <int NCT, int NBUF, int WG>
__device__ __forceinline__ void dense_ring_prologue(const float* w1hx, const int chunk_stride, const int wave, const int lane) {
#pragma unroll
    for (int c = 0; c < NBUF - 1; ++c) issue_chunk_uniform<NCT * 2, WG>(w1hx + (size_t)c * chunk_stride, hslot_at<NCT * 2 * 256, NBUF - 1>(c), wave, lane);
}

// the last step of a wave's statistics reduction, for the lane that holds the wave's hits and its largest key
__device__ __forceinline__ void dense_stats_commit(int* count, unsigned long long* key_out, const size_t at, const int hits, const unsigned long long key) {
    if (hits) atomicAdd(count + at, hits);
    if (key) atomicMax(key_out + at, key);
}

struct DenseParams {
    const float* feats;         // [B][..][96]: row 0 of window 0 of this group (the group's row offset t_max - T applied)
    long long seq_stride;       // floats from one sequence to the next
    int n_rows;                 // rows of a sequence from `feats` on
    int n_win, tiles;           // windows and tiles per sequence
    int T;
    const float* w1hx;          // the pass's first block of k-step 0 in the group's [T*3 ksteps][nets*4 ct][2 part][64][8 halves]
    int chunk_stride;           // floats from one k-step's chunk to the next (the whole group's chunk)
    HeadHxNet net[4];
    float* out;                 // [B][n_win][NL]
    int NL;
    int* range_flag;
    float fscale;
    // hit-mask mode (MASK): one word per wave and column instead of the matrix -- see the hit lists further down
    unsigned* mask;             // [NL][mask_col_stride] words; column c, sequence b, word k at c * mask_col_stride + b * mask_wps + k
    long long mask_col_stride;
    int mask_wps;               // words per sequence, ceil(n_win / 32)
    const float* thr;           // [NL]
};

// The hit word of one wave: tile t's 16 windows sit in lanes 0 .. 15 (j == 0), so the ballots' low halves side by side are the 32
// windows w0 + 32 wave .. + 31 in window order -- bit i = window 32 k + i of word k.  hit[t] must be false where the window does not exist.
__device__ __forceinline__ unsigned dense_hit_word(const bool hit0, const bool hit1) {
    return (unsigned)(__ballot(hit0) & 0xffffull) | ((unsigned)(__ballot(hit1) & 0xffffull) << 16);
}

template <int NN, int NBUF, int WG, bool MASK = false>
__global__ __launch_bounds__(64 * WG, 1) void heads_dense_kernel(DenseParams p) {
    using namespace owr;
    constexpr int NT = 2;                       // position tiles of 16 windows per wave, as heads_hx_kernel
    constexpr int TILE = 16 * NT * WG;
    constexpr int NCT = NN * 4;                 // hidden tiles of 16
    constexpr int NBLK = NCT * 2;               // 1 KB blocks per k-step chunk
    constexpr int CHUNK = NBLK * 256;           // floats
    constexpr int D = NBUF - 1;                 // chunks in flight ahead of the one being consumed
    constexpr int KDMA = NBLK / WG;             // DMA instructions per wave and chunk
    static_assert(NBLK % WG == 0 && (D - 1) * KDMA < 64, "the counted wait assumes the same issue count in every wave");
    extern __shared__ __attribute__((aligned(16))) float dense_rows[];
    const int lane = threadIdx.x & 63, pos = lane & 15, j = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KST = p.T * 3;                    // (>= 3 > D - 1: every prologue chunk exists)
    const int b = blockIdx.x / p.tiles, w0 = (blockIdx.x - b * p.tiles) * TILE;
    dense_ring_prologue<NCT, NBUF, WG>(p.w1hx, p.chunk_stride, wave, lane);
    dense_stage_rows<WG>(dense_rows, p.feats + (size_t)b * p.seq_stride, w0, p.n_rows, p.T, p.fscale);
    __syncthreads();                            // rows staged, prologue chunks landed (the fence drains them: once per tile)

    f32x4 acc[NCT][NT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B operand of k-step ks: position pos of tile t reads unit kstep_unit(ks, j) of staged row 16 (NT wave + t) + pos + ks / 3
    auto load_b = [&](int ks, Op (&bo)[NT]) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float* src = dense_rows + owd::unit_word(16 * (NT * wave + t) + pos + ks / 3, owd::kstep_unit(ks, j));
            bo[t].h = *reinterpret_cast<const f16x8*>(src);
            bo[t].l = *reinterpret_cast<const f16x8*>(src + 4);
        }
    };
    // The staged rows never change behind the prologue, so the B operand of k-step ks + 1 is read DURING k-step ks, beside its last
    // pair of hidden tiles, and is in registers when the barrier releases the waves -- as heads_hx_kernel's, whose split sits behind
    // the previous k-step's MFMAs.  Read at the top of its own k-step it put an LDS round trip in the open behind every barrier, for
    // all waves of the CU at once, 3 T times per tile.
    Op bcur[NT], bnext[NT];
    load_b(0, bcur);
    // one k-step: ring slot u (static), prefetch of k-step ks + D into slot (u + D) % NBUF, MFMAs, B operand of k-step ks + 1
    auto kstep = [&](int ks, auto uc, auto always) {
        constexpr int u = decltype(uc)::value;
        constexpr bool ALWAYS = decltype(always)::value;        // main loop: every k-step of the group prefetches and has a successor
        const float* cur = hslot_at<CHUNK, NBUF - 1>(u);
        if (ALWAYS || ks + D < KST) {                           // slot of k-step ks-1: every wave passed the last barrier
            constexpr int un = (u + D) % NBUF;
            issue_chunk_uniform<NBLK, WG>(p.w1hx + (size_t)(ks + D) * p.chunk_stride, hslot_at<CHUNK, NBUF - 1>(un), wave, lane);
        }
        // A operands one pair of hidden tiles ahead of their MFMAs, as heads_hx_kernel (OWH_HEADS_APIPE)
        f16x8 A[2][4];
#pragma unroll
        for (int bk = 0; bk < 4; ++bk) A[0][bk] = lds_h(cur, bk, lane);
#pragma unroll
        for (int c2 = 0; c2 < NCT; c2 += 2) {
            const int pc = (c2 / 2) & 1;
            if (c2 + 2 < NCT) {
#pragma unroll
                for (int bk = 0; bk < 4; ++bk) A[pc ^ 1][bk] = lds_h(cur, (c2 + 2) * 2 + bk, lane);
            } else if (ALWAYS || ks + 1 < KST) load_b(ks + 1, bnext);        // (flies under the last pair's MFMAs)
            __builtin_amdgcn_sched_barrier(0);                  // (the reads stay in front of this pair's MFMAs)
#pragma unroll
            for (int part = 0; part < 3; ++part) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    acc[c2][t] = OWH_MFMA(part == 2 ? A[pc][1] : A[pc][0], part == 1 ? bcur[t].l : bcur[t].h, acc[c2][t]);
                    acc[c2 + 1][t] = OWH_MFMA(part == 2 ? A[pc][3] : A[pc][2], part == 1 ? bcur[t].l : bcur[t].h, acc[c2 + 1][t]);
                }
            }
        }
        if (ALWAYS || ks + 1 < KST) {
            __builtin_amdgcn_sched_barrier(0);
            // this wave's part of chunk ks + 1 has landed when at most the chunks ks + 2 .. ks + D are outstanding
            if constexpr (ALWAYS) wait_vmcnt<(D - 1) * KDMA>();
            else wait_vmcnt<0>();
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // (lgkmcnt(0): this wave's reads of the slot, and bnext, have returned)
#pragma unroll
            for (int t = 0; t < NT; ++t) bcur[t] = bnext[t];
        }
    };
    auto group = [&](int ks0, auto always) {                    // NBUF consecutive k-steps, slots 0 .. NBUF-1
        constexpr bool ALWAYS = decltype(always)::value;
        static_for_while<0, NBUF>([&](auto uc) {
            constexpr int U = decltype(uc)::value;
            if (!ALWAYS && ks0 + U >= KST) return false;
            kstep(ks0 + U, uc, always);
            return true;
        });
    };
    int ks0 = 0;
    for (; ks0 + NBUF - 1 + D < KST; ks0 += NBUF) group(ks0, std::true_type{});
    for (; ks0 < KST; ks0 += NBUF) group(ks0, std::false_type{});        // the last D .. NBUF + D - 1 k-steps

    lanemask_t bad = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) nan_guard(bad, acc[0][t][0]);      // a feature beyond the f16 range
    float score[NN][NT];
#pragma unroll
    for (int n = 0; n < NN; ++n) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            f32x4 h1[4] = {acc[4 * n][t], acc[4 * n + 1][t], acc[4 * n + 2][t], acc[4 * n + 3][t]};
            score[n][t] = net64_score<NN>(p.net[n], h1, bad, j, lane);
        }
    }
    // ---- gating + store (one lane group per window: j == 0)
    if constexpr (MASK) {
        // the same gated value the matrix store would write, tested against the column's threshold: one plain store per wave and column
        const int word = (w0 + wave * 16 * NT) >> 5;           // (TILE and 16 NT are multiples of 32)
#pragma unroll
        for (int n = 0; n < NN; ++n) {
            if (p.net[n].role != 0) continue;
            const float thr = p.thr[p.net[n].out_col];
            bool hit[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int w = w0 + wave * 16 * NT + t * 16 + pos;
                float sc = score[n][t];
                if (n + 1 < NN && p.net[n + 1].role == 1 && p.net[n + 1].head == p.net[n].head && sc > 0.5f) sc = score[n + 1][t];
                hit[t] = j == 0 && w < p.n_win && sc >= thr;
            }
            const unsigned bits = dense_hit_word(hit[0], hit[1]);
            if (lane == 0 && word < p.mask_wps) p.mask[(size_t)p.net[n].out_col * p.mask_col_stride + (size_t)b * p.mask_wps + word] = bits;
        }
    } else if (j == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int w = w0 + wave * 16 * NT + t * 16 + pos;
            if (w >= p.n_win) continue;
            float* o = p.out + ((size_t)b * p.n_win + w) * p.NL;
#pragma unroll
            for (int n = 0; n < NN; ++n) {
                if (p.net[n].role != 0) continue;
                float sc = score[n][t];
                if (n + 1 < NN && p.net[n + 1].role == 1 && p.net[n + 1].head == p.net[n].head && sc > 0.5f) sc = score[n + 1][t];
                o[p.net[n].out_col] = sc;
            }
        }
    }
    raise_range_flag(bad, p.range_flag);        // (position unknown: a window is no stream)
}

// windows [first, first + n) of the flattened [B][n_win] window list -> slab [n][T][96]; one 16-byte piece per thread and turn
struct GatherParams {
    const float* feats;         // the head's row offset applied
    long long seq_stride;       // floats
    long long n_win, first, n;
    int T;
    float* slab;
};
__global__ void dense_gather_kernel(GatherParams p) {
    const long long per = (long long)p.T * 24, total = p.n * per;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long win = i / per, q = i - win * per;
        const long long gw = p.first + win, b = gw / p.n_win, w = gw - b * p.n_win;
        reinterpret_cast<owr::f32x4*>(p.slab)[i] = *reinterpret_cast<const owr::f32x4*>(p.feats + b * p.seq_stride + w * 96 + q * 4);
    }
}

// ---- dense scoring over the head bank (include/owwhip.h: oww_bank_score_features, oww_bank_score_stats) --------------
// heads_dense_bank_kernel<NBUF, WG>: heads_dense_kernel<1, NBUF, WG> with the head a loop variable.  ONE launch covers every listed
// narrow bank head (HT = 4): block = (head slice, sequence, tile) (owd::bank_plan), and a workgroup stages its tile's rows once -- the
// rows of the LONGEST head of the launch, t_s: 32 WG + t_s - 1 of them from row w0 + t_max - t_s on (dense_stage_rows) -- and then
// walks the hpw heads of its slice, each with its own BankHeadDev (w1hx, net, T) from the handle's bank:
//  * a head of length T reads its own last T rows of every window: its k-step ks takes the B operand from staged row
//    16 (2 wave + t) + pos + (t_s - T) + ks / 3 (owd::bank_staged_row), then the same MFMA triplets in the same order and net64_score<1>,
//    so a score is bit for bit heads_bank_kernel's, and with it the fixed heads kernel's, for the materialised window.
//  * hand-over of the ring.  A head's k loop ends without a barrier, and the next head's prologue refills slots 0 .. D-1, one of which
//    the slowest wave may still be reading: so lgkmcnt(0) + a bare s_barrier first, then the next head's first D chunks are issued --
//    under this head's tail (net64_score, the store or the reduction), which covers their L2 round trip -- and the next head begins
//    with vmcnt(0) + __syncthreads(): the chunks have landed in every wave and the tail's stores and atomics have retired, which is
//    the k loop's entry condition (the head of this file).  Inside a head the discipline is heads_dense_kernel's, unchanged.
//  * matrix mode (out != nullptr): out[b][w][col] = score.  Statistics mode: count of scores >= thr[col], and the maximum with the
//    first window that attains it as ONE integer key (owd::stat_key) -- reduced over the wave's 32 windows in registers, then one
//    atomicAdd and one 64-bit atomicMax per wave and head.  Integer atomics commute: the result does not depend on scheduling.
struct DenseBankItem { int head, col; };       // bank id, column of the caller's list
struct DenseBankParams {
    const float* feats;         // [B][..][96]: first staged row of window 0 (the launch's row offset t_max - t_s applied)
    long long seq_stride;       // floats from one sequence to the next
    int n_rows;                 // rows of a sequence from `feats` on
    int n_win, seq_tiles, tiles;    // windows and tiles per sequence; B x seq_tiles
    int t_s;                    // the largest T of the launch's heads
    const BankHeadDev* heads;   // the handle's bank
    const DenseBankItem* items; // [n_items] the launch's heads
    int n_items, hpw;
    float* out;                 // [B][n_win][n_ids], or nullptr = statistics
    int n_ids;
    const float* thr;           // [n_ids]
    int* count;                 // [B][n_ids]
    unsigned long long* key;    // [B][n_ids]
    int* range_flag;
    float fscale;
    // hit-mask mode (MASK), as DenseParams: column = it.col, thresholds = thr
    unsigned* mask;             // [n_ids][mask_col_stride]
    long long mask_col_stride;
    int mask_wps;
};

template <int NBUF, int WG, bool MASK = false>
__global__ __launch_bounds__(64 * WG, 1) void heads_dense_bank_kernel(DenseBankParams p) {
    using namespace owr;
    constexpr int NT = 2;
    constexpr int TILE = 16 * NT * WG;
    constexpr int NCT = 4;                      // one narrow net
    constexpr int NBLK = NCT * 2;
    constexpr int CHUNK = NBLK * 256;
    constexpr int D = NBUF - 1;
    constexpr int KDMA = NBLK / WG;
    static_assert(NBLK % WG == 0 && (D - 1) * KDMA < 64, "the counted wait assumes the same issue count in every wave");
    extern __shared__ __attribute__((aligned(16))) float dense_rows[];
    const int lane = threadIdx.x & 63, pos = lane & 15, j = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slice = owd::bank_block_slice(blockIdx.x, p.tiles), tile = owd::bank_block_tile(blockIdx.x, p.tiles);
    const int b = tile / p.seq_tiles, w0 = (tile - b * p.seq_tiles) * TILE;
    const int i0 = owd::bank_slice_first(slice, p.hpw), nh = owd::bank_slice_count(slice, p.hpw, p.n_items);
    dense_ring_prologue<NCT, NBUF, WG>(p.heads[p.items[i0].head].w1hx, CHUNK, wave, lane);
    dense_stage_rows<WG>(dense_rows, p.feats + (size_t)b * p.seq_stride, w0, p.n_rows, p.t_s, p.fscale);       // once for all heads of the slice

    lanemask_t bad = 0;
    for (int r = 0; r < nh; ++r) {
        const DenseBankItem it = p.items[i0 + r];
        const BankHeadDev* hd = p.heads + it.head;
        const float* w1hx = hd->w1hx;
        const int T = hd->T, KST = T * 3;
        // this head's first D chunks have landed in every wave, the last head's stores and atomics have retired (and, r = 0, the rows
        // are staged): the k loop starts with nothing outstanding
        wait_vmcnt<0>();
        __syncthreads();

        f32x4 acc[NCT][NT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto load_b = [&](int ks, Op (&bo)[NT]) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float* src = dense_rows + owd::unit_word(owd::bank_staged_row(wave, t, pos, p.t_s, T, ks), owd::kstep_unit(ks, j));
                bo[t].h = *reinterpret_cast<const f16x8*>(src);
                bo[t].l = *reinterpret_cast<const f16x8*>(src + 4);
            }
        };
        Op bcur[NT], bnext[NT];
        load_b(0, bcur);
        // one k-step, as heads_dense_kernel<1>: ring slot u (static), prefetch of k-step ks + D, MFMAs, B operand of k-step ks + 1
        auto kstep = [&](int ks, auto uc, auto always) {
            constexpr int u = decltype(uc)::value;
            constexpr bool ALWAYS = decltype(always)::value;
            const float* cur = hslot_at<CHUNK, NBUF - 1>(u);
            if (ALWAYS || ks + D < KST) {                           // slot of k-step ks-1: every wave passed the last barrier
                constexpr int un = (u + D) % NBUF;
                issue_chunk_uniform<NBLK, WG>(w1hx + (size_t)(ks + D) * CHUNK, hslot_at<CHUNK, NBUF - 1>(un), wave, lane);
            }
            f16x8 A[2][4];
#pragma unroll
            for (int bk = 0; bk < 4; ++bk) A[0][bk] = lds_h(cur, bk, lane);
#pragma unroll
            for (int c2 = 0; c2 < NCT; c2 += 2) {
                const int pc = (c2 / 2) & 1;
                if (c2 + 2 < NCT) {
#pragma unroll
                    for (int bk = 0; bk < 4; ++bk) A[pc ^ 1][bk] = lds_h(cur, (c2 + 2) * 2 + bk, lane);
                } else if (ALWAYS || ks + 1 < KST) load_b(ks + 1, bnext);        // (flies under the last pair's MFMAs)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int part = 0; part < 3; ++part) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        acc[c2][t] = OWH_MFMA(part == 2 ? A[pc][1] : A[pc][0], part == 1 ? bcur[t].l : bcur[t].h, acc[c2][t]);
                        acc[c2 + 1][t] = OWH_MFMA(part == 2 ? A[pc][3] : A[pc][2], part == 1 ? bcur[t].l : bcur[t].h, acc[c2 + 1][t]);
                    }
                }
            }
            if (ALWAYS || ks + 1 < KST) {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (ALWAYS) wait_vmcnt<(D - 1) * KDMA>();
                else wait_vmcnt<0>();
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
                for (int t = 0; t < NT; ++t) bcur[t] = bnext[t];
            }
        };
        auto group = [&](int ks0, auto always) {
            constexpr bool ALWAYS = decltype(always)::value;
            static_for_while<0, NBUF>([&](auto uc) {
                constexpr int U = decltype(uc)::value;
                if (!ALWAYS && ks0 + U >= KST) return false;
                kstep(ks0 + U, uc, always);
                return true;
            });
        };
        int ks0 = 0;
        for (; ks0 + NBUF - 1 + D < KST; ks0 += NBUF) group(ks0, std::true_type{});
        for (; ks0 < KST; ks0 += NBUF) group(ks0, std::false_type{});

        // ---- hand-over: every wave's reads of the last slots have returned before the next head's prologue refills slots 0 .. D-1
        if (r + 1 < nh) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            dense_ring_prologue<NCT, NBUF, WG>(p.heads[p.items[i0 + r + 1].head].w1hx, CHUNK, wave, lane);
        }

        // ---- tail (the next head's first chunks fly under it)
#pragma unroll
        for (int t = 0; t < NT; ++t) nan_guard(bad, acc[0][t][0]);
        const HeadHxNet net = hd->net;
        float score[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            f32x4 h1[4] = {acc[0][t], acc[1][t], acc[2][t], acc[3][t]};
            score[t] = net64_score<1>(net, h1, bad, j, lane);
        }
        if constexpr (MASK) {
            const float thr = p.thr[it.col];
            const int word = (w0 + wave * 16 * NT) >> 5;
            bool hit[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) hit[t] = j == 0 && w0 + wave * 16 * NT + t * 16 + pos < p.n_win && score[t] >= thr;
            const unsigned bits = dense_hit_word(hit[0], hit[1]);
            if (lane == 0 && word < p.mask_wps) p.mask[(size_t)it.col * p.mask_col_stride + (size_t)b * p.mask_wps + word] = bits;
        } else if (p.out) {
            if (j == 0) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int w = w0 + wave * 16 * NT + t * 16 + pos;
                    if (w < p.n_win) p.out[((size_t)b * p.n_win + w) * p.n_ids + it.col] = score[t];
                }
            }
        } else {
            const float thr = p.thr[it.col];
            int hits = 0;
            unsigned long long key = 0ull;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int w = w0 + wave * 16 * NT + t * 16 + pos;
                const bool valid = j == 0 && w < p.n_win;
                hits += __popcll(__ballot(valid && score[t] >= thr));
                if (valid) {
                    const unsigned long long k = owd::stat_key(__float_as_uint(score[t]), (unsigned)w);
                    key = k > key ? k : key;
                }
            }
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {                  // lanes 0..15 carry the wave's windows (j == 0), the others 0
                const unsigned long long o = __shfl_xor(key, m);
                key = o > key ? o : key;
            }
            if (lane == 0) dense_stats_commit(p.count, p.key, (size_t)b * p.n_ids + it.col, hits, key);
        }
    }
    raise_range_flag(bad, p.range_flag);        // (position unknown: a window is no stream)
}

// The fallback's last step: the scores of one slab (windows [first, first + n) of the flattened [B][n_win] list, one bank head, as
// heads_bank_kernel left them in its ext mode) -> column `col` of the matrix, or into the statistics with the keys of the kernel above.
// A wave whose windows lie in one sequence reduces in registers first; one that straddles two sequences lets every lane speak.
struct BankSlabParams {
    const float* scores;        // [n]
    long long n_win, first, n;
    float* out; int n_ids, col;
    float thr; int* count; unsigned long long* key;
};
__global__ void dense_bank_slab_kernel(BankSlabParams p) {
    const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) & ~63ll;        // the wave's first window of the slab
    if (i0 >= p.n) return;
    const long long i = i0 + (threadIdx.x & 63);
    const bool valid = i < p.n;
    const long long gw = p.first + (valid ? i : p.n - 1), b = gw / p.n_win, w = gw - b * p.n_win;
    const float sc = p.scores[valid ? i : p.n - 1];
    if (p.out) {
        if (valid) p.out[(size_t)gw * p.n_ids + p.col] = sc;
        return;
    }
    const long long b_first = (p.first + i0) / p.n_win, b_last = (p.first + min(i0 + 63, p.n - 1)) / p.n_win;
    unsigned long long key = valid ? owd::stat_key(__float_as_uint(sc), (unsigned)w) : 0ull;
    const bool hit = valid && sc >= p.thr;
    const size_t at = (size_t)b * p.n_ids + p.col;
    if (b_first == b_last) {
        const int hits = __popcll(__ballot(hit));
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned long long o = __shfl_xor(key, m);
            key = o > key ? o : key;
        }
        if ((threadIdx.x & 63) == 0) dense_stats_commit(p.count, p.key, at, hits, key);
    } else if (valid) {
        if (hit) atomicAdd(p.count + at, 1);
        atomicMax(p.key + at, key);
    }
}

// ---- ordered hit lists (include/owwhip.h: oww_score_hits, oww_score_clip_hits, oww_bank_score_hits) ------------------
// The sliding kernels' MASK mode leaves one bit per (column, sequence, window) -- mask[col][seq][w / 32], bit w % 32, written with
// plain stores, one word per wave and column -- and the kernels below turn the mask into the caller's lists
// (owwhip_dense_hits_host.h states the geometry and, in owdh::compact, what the compaction computes):
//  * dense_hits_slab_kernel     the fallback forms: the scores of one gathered slab -> the same bits.  A slab starts and ends anywhere
//                               in a word, so the bits are ORed in (integer atomics commute; the column's words are cleared first).
//  * dense_hits_compact_kernel  one workgroup per column walks the column's words in (seq, word) order, 1,024 words a turn (one
//                               16-byte load per thread), with a running offset -- popcount, workgroup scan, carry -- writes set bit
//                               number r as a record (seq, window, 0, 0) to slot r while r < cap, and the column's total as a 64-bit
//                               count.  No atomics: slot r is a function of the mask alone.
//  * dense_hits_gather_kernel   dense_gather_kernel with the window taken from the list: the head's own T rows of n stored hits ->
//                               slab [n][T][96], one 16-byte piece per thread and turn.
//  * dense_hits_score_kernel    the re-scored slab's scores (heads_bank_kernel / run_heads on external features, the bits of the
//                               matrix entry) into the records.
struct HitSlabParams {
    const float* scores;        // score of slab window i at scores[i * stride + off]
    int stride, off;
    long long n_win, first, n;  // windows [first, first + n) of the flattened [B][n_win] list
    float thr;
    unsigned* mask;             // the column's words [B][wps]
    long long wps;
};
__global__ void dense_hits_slab_kernel(HitSlabParams p) {
    // A wave holds 64 consecutive windows of the flattened list.  The lanes of one mask word are consecutive, and the word's first lane
    // -- the lane of bit 0, or lane 0 where the wave starts inside a word -- ORs in the whole word's share of the wave's ballot: one
    // atomic per word instead of one per hit.  A word ends with its 32nd bit or with its sequence, whichever comes first.
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < p.n;
    const long long gw = p.first + (valid ? i : p.n - 1), b = gw / p.n_win, w = gw - b * p.n_win;
    const unsigned long long hits = __ballot(valid && p.scores[(size_t)(valid ? i : p.n - 1) * p.stride + p.off] >= p.thr);
    const int bit0 = (int)(w & 31);
    if (!valid || (bit0 != 0 && lane != 0)) return;
    const long long left = p.n_win - w;                            // windows of this sequence from w on
    const int count = (int)(left < 32 - bit0 ? left : 32 - bit0);  // lanes of this word from this lane on (lanes beyond the slab voted 0)
    const unsigned bits = ((unsigned)(hits >> lane) & (count == 32 ? 0xffffffffu : (1u << count) - 1u)) << bit0;
    if (bits) atomicOr(p.mask + b * p.wps + (w >> 5), bits);
}

struct HitCompactParams {
    const unsigned* mask;       // [n_cols][col_stride]; col_stride a multiple of 4 words (16-byte loads)
    long long col_stride, wps;
    int B, cap;                 // cap: slots per column of `hits`
    int4* hits;                 // [n_cols][cap] records (seq, window, score bits = 0, reserved = 0)
    unsigned long long* total;  // [n_cols]
};
__global__ __launch_bounds__(256) void dense_hits_compact_kernel(HitCompactParams p) {
    __shared__ unsigned wave_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned* m = p.mask + (size_t)blockIdx.x * p.col_stride;
    int4* out = p.hits + (size_t)blockIdx.x * p.cap;
    const long long words = (long long)p.B * p.wps;
    unsigned long long carry = 0;               // set bits of the words in front of this turn
    for (long long base = 0; base < words; base += 1024) {
        const long long i4 = base + tid * 4;
        unsigned v[4] = {0u, 0u, 0u, 0u};
        if (i4 < words) {                       // (i4 + 3 < col_stride: the column is padded to four words)
            const uint4 q = *reinterpret_cast<const uint4*>(m + i4);
            v[0] = q.x; v[1] = i4 + 1 < words ? q.y : 0u; v[2] = i4 + 2 < words ? q.z : 0u; v[3] = i4 + 3 < words ? q.w : 0u;
        }
        const unsigned cnt = __popc(v[0]) + __popc(v[1]) + __popc(v[2]) + __popc(v[3]);
        unsigned inc = cnt;                     // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        unsigned before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { before += k < wave ? wave_sum[k] : 0u; all += wave_sum[k]; }
        unsigned long long r = carry + before + (inc - cnt);
        if (cnt && r < (unsigned long long)p.cap) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned bits = v[k];
                const long long idx = i4 + k, seq = idx / p.wps, w32 = (idx - seq * p.wps) * 32;
                while (bits && r < (unsigned long long)p.cap) {
                    const int bit = __ffs(bits) - 1;
                    out[r] = make_int4((int)seq, (int)(w32 + bit), 0, 0);
                    bits &= bits - 1; ++r;
                }
                r += __popc(bits);              // (only where the cap cut the word short)
            }
        }
        carry += all;
        __syncthreads();                        // (wave_sum is rewritten in the next turn)
    }
    if (tid == 0) p.total[blockIdx.x] = carry;
}

struct HitGatherParams {
    const float* feats;         // the head's row offset applied
    long long seq_stride;       // floats
    const int4* hits;           // [n] records of the slab's windows
    long long n;
    int T;
    float* slab;                // [n][T][96]
};
__global__ void dense_hits_gather_kernel(HitGatherParams p) {
    const long long per = (long long)p.T * 24, total = p.n * per;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long win = i / per, q = i - win * per;
        const int4 hit = p.hits[win];
        reinterpret_cast<owr::f32x4*>(p.slab)[i] = *reinterpret_cast<const owr::f32x4*>(p.feats + hit.x * p.seq_stride + (long long)hit.y * 96 + q * 4);
    }
}

struct HitScoreParams {
    const float* scores;        // score of slab window i at scores[i * stride + off]
    int stride, off;
    long long n;
    int4* hits;                 // [n]
};
__global__ void dense_hits_score_kernel(HitScoreParams p) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < p.n) p.hits[i].z = __float_as_int(p.scores[(size_t)i * p.stride + p.off]);
}

}  // namespace owh
