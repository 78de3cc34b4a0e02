// owwhip_state.h -- stream state records (oww_state_export / oww_state_import / oww_move_streams): a gather kernel pair
// (live layouts -> records) and a scatter kernel pair (records -> live layouts).  Pure data movement; the only roof is HBM.
//
// Record of one stream (words of 4 bytes, copied as bits; every section starts on a 16-byte boundary and is padded to one):
//   [header 8 words] [flat sections ...] [grouped sections ...]
// * header: magic, layout version, record bytes, 0, fingerprint (low, high), 0, 0.
// * flat section: an array in which the stream's words are contiguous (live + stream * stride): the spg = 1 conv histories, the
//   PCM tail, the feature and score rings, counters, raw / final scores, VAD ring, bank slot outputs.  One thread moves one 16-byte
//   quad of the record; the live side is a 16-byte access as well where the stream's stride keeps it aligned.
// * grouped section: an array kept in blocks of SPG streams in register-dump order [...][16 positions]; of every run of 16 words
//   the stream owns PPR: position m * SPG + p (interleaved, the f16-split family and the VAD (h, c) tiles) or p * PPR + m (the fp32
//   family) for its place p in the group -- the map owk::reset_kernel and owv::vad_reset_kernel walk.  The record holds the stream's
//   words in ascending block index, so a record leaves place p of one group and enters place q of another.  One workgroup serves
//   one (group block, array): a thread reads whole runs with 16-byte loads and writes each listed stream's words as 16-byte quads;
//   scattering, a block all of whose streams are listed is written as full rows, any other with plain 4-byte stores to the listed
//   streams' own lanes only -- no word of another stream is read, modified or written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "owwhip_state_host.h"     // kMagic, kLayoutVersion, kHeaderWords, FlatSection

namespace ows {

struct FlatParams {
    const int* ids;                // [n] live stream of record i
    const FlatSection* sec;        // [n_sec], ascending off
    int n_sec;
    uint32_t flat_quads;           // header + flat sections, in 16-byte quads
    uint32_t* rec;                 // records
    uint32_t record_words;
    uint32_t record_bytes;
    uint32_t fp_lo, fp_hi;
};

// grid (n records, ceil(flat_quads / 256)), 256 threads: thread = one quad of one record
template <bool SCATTER>
__global__ __launch_bounds__(256) void state_flat_kernel(FlatParams p) {
    const uint32_t q = blockIdx.y * 256u + threadIdx.x;
    if (q >= p.flat_quads) return;
    const int s = p.ids[blockIdx.x];
    uint4* rq = reinterpret_cast<uint4*>(p.rec + (size_t)blockIdx.x * p.record_words) + q;
    const uint32_t w = q * 4u;
    if (w < (uint32_t)kHeaderWords) {
        if (!SCATTER) *rq = q == 0 ? make_uint4(kMagic, kLayoutVersion, p.record_bytes, 0u) : make_uint4(p.fp_lo, p.fp_hi, 0u, 0u);
        return;
    }
    int k = 0;
    while (k + 1 < p.n_sec && w >= p.sec[k + 1].off) ++k;
    const FlatSection sc = p.sec[k];
    const uint32_t e = w - sc.off;
    uint32_t* lv = sc.live + (size_t)s * sc.stride + e;
    if (sc.vec) {
        if (SCATTER) *reinterpret_cast<uint4*>(lv) = *rq;
        else *rq = *reinterpret_cast<const uint4*>(lv);
    } else if (SCATTER) {
        const uint4 v = *rq;
        if (e < sc.len) lv[0] = v.x;
        if (e + 1 < sc.len) lv[1] = v.y;
        if (e + 2 < sc.len) lv[2] = v.z;
        if (e + 3 < sc.len) lv[3] = v.w;
    } else {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (e < sc.len) v.x = lv[0];
        if (e + 1 < sc.len) v.y = lv[1];
        if (e + 2 < sc.len) v.z = lv[2];
        if (e + 3 < sc.len) v.w = lv[3];
        *rq = v;
    }
}

struct GroupParams {
    uint32_t* live;            // first group block
    uint32_t block_words;      // words per group block (a multiple of 16 * runs per thread)
    const int* items;          // [n_groups][1 + SPG]: group index, then the record index of each place (-1 = not listed)
    int n_chunks;              // threads' worth of work per block: block_words / (16 * runs per thread)
    uint32_t* rec;
    uint32_t record_words;
    uint32_t off;              // word offset of the section in the record
};

// grid (n_groups, ceil(n_chunks / 64)), 64 threads: thread = R consecutive runs of one group block, R * PPR = a multiple of 4 words
template <int SPG, int PPR, bool IL, bool SCATTER>
__global__ __launch_bounds__(64) void state_group_kernel(GroupParams p) {
    constexpr int R = PPR >= 4 ? 1 : 4 / PPR;
    constexpr int NW = R * PPR;                      // record words per stream and thread: 8 or 4
    constexpr bool COVERED = SPG * PPR == 16;        // every lane of a run belongs to a stream
    static_assert(NW % 4 == 0 && SPG * PPR <= 16, "quads on the record side");
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (c >= p.n_chunks) return;
    const int* it = p.items + (size_t)blockIdx.x * (1 + SPG);
    int rec[SPG];
    bool full = COVERED;
#pragma unroll
    for (int sp = 0; sp < SPG; ++sp) { rec[sp] = it[1 + sp]; full = full && rec[sp] >= 0; }
    uint32_t* lv = p.live + (size_t)it[0] * p.block_words + (size_t)c * (R * 16);
    uint32_t v[R * 16];
    if (!SCATTER) {
#pragma unroll
        for (int i = 0; i < R * 4; ++i) {
            const uint4 t = reinterpret_cast<const uint4*>(lv)[i];
            v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
        }
#pragma unroll
        for (int sp = 0; sp < SPG; ++sp) {
            if (rec[sp] < 0) continue;
            uint4* out = reinterpret_cast<uint4*>(p.rec + (size_t)rec[sp] * p.record_words + p.off + (size_t)c * NW);
            uint32_t o[NW];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int m = 0; m < PPR; ++m) o[r * PPR + m] = v[r * 16 + (IL ? m * SPG + sp : sp * PPR + m)];
#pragma unroll
            for (int i = 0; i < NW / 4; ++i) out[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
        }
    } else {
#pragma unroll
        for (int sp = 0; sp < SPG; ++sp) {
            if (rec[sp] < 0) continue;
            const uint4* in = reinterpret_cast<const uint4*>(p.rec + (size_t)rec[sp] * p.record_words + p.off + (size_t)c * NW);
            uint32_t o[NW];
#pragma unroll
            for (int i = 0; i < NW / 4; ++i) { const uint4 t = in[i]; o[4 * i] = t.x; o[4 * i + 1] = t.y; o[4 * i + 2] = t.z; o[4 * i + 3] = t.w; }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int m = 0; m < PPR; ++m) {
                    const int at = r * 16 + (IL ? m * SPG + sp : sp * PPR + m);
                    if (full) v[at] = o[r * PPR + m];
                    else lv[at] = o[r * PPR + m];              // the stream's own lane, nothing else
                }
        }
        if (full) {
#pragma unroll
            for (int i = 0; i < R * 4; ++i) reinterpret_cast<uint4*>(lv)[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
        }
    }
}

}  // namespace ows
