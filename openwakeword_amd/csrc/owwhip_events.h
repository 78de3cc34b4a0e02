// owwhip_events.h -- detections as ordered device-side events with feature snapshots (include/owwhip.h: oww_events_*).
//
// After a step every (stream, fixed score column) and (stream, subscribed bank slot) pair whose post-processed score reaches its event
// threshold becomes one 32-byte oww_event record, in ascending (stream, column, slot) order, with the stream's last feature rows copied
// beside it -- in the step that detected, before a later step moves the ring.  Two launches on the handle's stream, gfx950, wave64:
//   events_count_kernel  one thread per pair (stream-major, NL + K pairs per stream), 256 per workgroup: hit predicate, wave ballot,
//                        one popcount per workgroup into block_count[n_blocks]
//   events_write_kernel  same grid: a workgroup's first rank = the sum of the block counts before it (strided reduction over
//                        block_count with all 256 threads), rank inside the workgroup from the ballot + mbcnt; hits of rank < capacity
//                        store their record (two 16-byte stores) and the workgroup copies their feature rows in one flat walk (16-byte
//                        accesses, a 384-byte row per 24 lanes); workgroup 0 sums every block count and stores {min(total, capacity), total}
// No atomics and no waiting between workgroups: the order comes from the launch boundary between the two kernels.  Every record and
// snapshot store is bounded by `capacity` here, whatever the host passed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "owwhip.h"

namespace owe {

constexpr int EV_WG = 256;                    // threads (pairs) per workgroup: four waves
constexpr int EV_ROW_QUADS = OWW_EMB_DIM / 4; // 16-byte pieces of one feature row

struct EventsParams {
    const float* scores;          // [S][NL] post-processed scores of the call (d_scores)
    const float* bank_scores;     // [S][K] post-processed bank scores; unused when K == 0
    const int* bank_sub;          // [S][K] live subscription table, -1 = empty slot
    const float* thr_fixed;       // [NL] event thresholds, NaN = the column never reports
    float thr_bank;               // event threshold of every bank slot
    const uint8_t* stream_on;     // masked call: [S] 1 = the stream took part; nullptr = all did
    const uint32_t* npred;        // [S] prediction counters after the call (oww_event::frame)
    const uint32_t* nfeat;        // [S] feature ring counters after the call
    const float* feat;            // [S][TR][96] feature rings
    int TR, NL, K;
    int n_pairs;                  // S * (NL + K)
    int n_blocks;                 // workgroups of both launches
    int* block_count;             // [n_blocks] hits per workgroup (count kernel -> write kernel)
    oww_event* rec;               // [capacity] records
    int* count;                   // {n_stored, n_total}
    float* snap;                  // [capacity][rows][96] feature snapshots; unused when rows == 0
    int capacity, rows;
};

// The hit predicate of pair i: the stream took part, the pair exists (a fixed column, or a slot with a subscription) and its
// post-processed score is >= its event threshold (false for a NaN threshold).
__device__ __forceinline__ bool event_hit(const EventsParams& p, int i, int& s, int& j, float& sc) {
    s = 0; j = 0; sc = 0.0f;
    if (i >= p.n_pairs) return false;
    const int P = p.NL + p.K;
    s = i / P;
    j = i - s * P;
    if (p.stream_on && !p.stream_on[s]) return false;
    float thr;
    if (j < p.NL) {
        sc = p.scores[(size_t)s * p.NL + j];
        thr = p.thr_fixed[j];
    } else {
        const size_t k = (size_t)s * p.K + (j - p.NL);
        if (p.bank_sub[k] < 0) return false;
        sc = p.bank_scores[k];
        thr = p.thr_bank;
    }
    return sc >= thr;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(EV_WG) void events_count_kernel(EventsParams p) {
    __shared__ int wave_hits[EV_WG / 64];
    int s, j;
    float sc;
    const bool hit = event_hit(p, blockIdx.x * EV_WG + threadIdx.x, s, j, sc);
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0) wave_hits[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) p.block_count[blockIdx.x] = wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
}

__global__ __launch_bounds__(EV_WG) void events_write_kernel(EventsParams p) {
    __shared__ int wave_part[EV_WG / 64];
    __shared__ int wave_hits[EV_WG / 64];
    __shared__ int hit_stream[EV_WG];          // stream of the workgroup's stored hits, by rank inside the workgroup
    __shared__ uint32_t hit_cnt[EV_WG];        // ... and its feature ring counter
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // first rank of this workgroup = hits of the workgroups before it; workgroup 0 (first rank 0) sums all of them for the total
    const int n_sum = blockIdx.x == 0 ? p.n_blocks : (int)blockIdx.x;
    int part = 0;
    for (int b = tid; b < n_sum; b += EV_WG) part += p.block_count[b];
    part = wave_sum(part);
    int s, j;
    float sc;
    const bool hit = event_hit(p, blockIdx.x * EV_WG + tid, s, j, sc);
    const unsigned long long m = __ballot(hit);
    if (lane == 0) { wave_part[wave] = part; wave_hits[wave] = __popcll(m); }
    __syncthreads();
    const int sum = wave_part[0] + wave_part[1] + wave_part[2] + wave_part[3];
    const int base = blockIdx.x == 0 ? 0 : sum;
    if (blockIdx.x == 0 && tid == 0) { p.count[0] = sum < p.capacity ? sum : p.capacity; p.count[1] = sum; }
    int local = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));   // hits in lower lanes
    for (int w = 0; w < wave; ++w) local += wave_hits[w];
    const int room = p.capacity - base;        // ranks base .. base + room - 1 are stored (ranks ascend inside the workgroup)
    if (hit && local < room) {
        const int rank = base + local;
        int4 lo, hi;
        lo.x = s;
        lo.y = j < p.NL ? j : ~(j - p.NL);
        lo.z = j < p.NL ? -1 : p.bank_sub[(size_t)s * p.K + (j - p.NL)];
        lo.w = __float_as_int(sc);
        hi.x = (int)p.npred[s];
        hi.y = p.rows > 0 ? rank : -1;
        hi.z = 0; hi.w = 0;
        int4* out = reinterpret_cast<int4*>(p.rec + rank);
        out[0] = lo;
        out[1] = hi;
        hit_stream[local] = s;
        hit_cnt[local] = p.nfeat[s];
    }
    if (p.rows <= 0) return;
    __syncthreads();
    const int total = wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
    const int n_stored = room <= 0 ? 0 : (total < room ? total : room);
    // The stored hits' blocks are contiguous in snap (ranks base .. base + n_stored - 1): one flat walk over their 16-byte pieces,
    // four independent loads in flight per thread -- when a call overflows, the stored hits crowd into the first few workgroups and
    // a hit-by-hit walk would pay a dependent load chain per hit.  After the call the newest row of a ring sits at slot
    // (cnt - 1) % TR (oww_get_features); piece e of a block is row e / 24 (oldest first), columns 4 (e % 24) .. + 3.
    const int quads = p.rows * EV_ROW_QUADS;
    const int n_el = n_stored * quads;
    const uint32_t back = (uint32_t)(2 * p.TR - p.rows);
    const float4* feat4 = reinterpret_cast<const float4*>(p.feat);
    float4* dst = reinterpret_cast<float4*>(p.snap) + (size_t)base * quads;
    auto piece = [&](int idx) {
        const int q = idx / quads, e = idx - q * quads;
        const int t = e / EV_ROW_QUADS, c = e - t * EV_ROW_QUADS;
        const uint32_t slot = (hit_cnt[q] + back + (uint32_t)t) % (uint32_t)p.TR;
        return feat4 + ((size_t)hit_stream[q] * p.TR + slot) * EV_ROW_QUADS + c;
    };
    int idx = tid;
    for (; idx + 3 * EV_WG < n_el; idx += 4 * EV_WG) {
        const float4 v0 = *piece(idx), v1 = *piece(idx + EV_WG), v2 = *piece(idx + 2 * EV_WG), v3 = *piece(idx + 3 * EV_WG);
        dst[idx] = v0; dst[idx + EV_WG] = v1; dst[idx + 2 * EV_WG] = v2; dst[idx + 3 * EV_WG] = v3;
    }
    for (; idx < n_el; idx += EV_WG) dst[idx] = *piece(idx);
}

}  // namespace owe
