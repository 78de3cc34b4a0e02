// owwhip_audio.h -- each stream's recent 16 kHz audio on the device (include/owwhip.h: oww_audio_configure, oww_get_audio,
// oww_get_event_audio): the ring int16 [S][ring_chunks][1280] with one uint32 chunk counter per stream, what the reference keeps as
// AudioFeatures.raw_data_buffer (utils.py:164,174,407).  Three kernels, gfx950, wave64, pure data movement in 16-byte pieces (a chunk is
// 160 of them); the index map is owwhip_audio_host.h's, the same functions the host program tests:
//   audio_append_kernel  one wave owns one stream, four waves per workgroup.  Every lane reads the stream's counter, the wave copies
//                        the call's kept chunks (the last min(k, ring_chunks)) into slots (counter + c) % ring_chunks with four
//                        independent loads in flight per lane, then lane 0 stores counter + k.  The ownership is what makes the counter
//                        safe: no other wave of the launch reads or writes this stream's counter or ring.  Honours a participation mask
//                        and a participant list (masked steps).  Without a source it is oww_reset's: the listed streams' rings and
//                        counters become zero.
//   audio_gather_kernel  oww_get_audio: grid (listed stream, chunk), one wave per chunk: ring -> dense rows, oldest chunk first, zeros
//                        for the chunks the stream has not received since its reset; the wave of chunk 0 stores the stream's counter.
//   events_audio_kernel  behind events_write_kernel: a grid sized to the chip walks the n_stored x event_chunks chunk copies of the
//                        call, one wave per copy, grid stride.  Reads {n_stored} and the records' streams from the device; bounded by
//                        `capacity` here, whatever the count word holds.
// No atomics and no waiting between workgroups.  The ring side and every destination are 16-byte aligned; the append's source is the
// caller's PCM (oww_step takes any alignment of a device pointer; the row stride, k x 2,560 bytes, is always a multiple of 16): a base
// that is not 16-byte aligned takes element-wise loads.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "owwhip.h"
#include "owwhip_audio_host.h"

namespace owa {

constexpr int AU_WG = 256;                     // four waves: four streams (append) per workgroup
constexpr int AU_EVENT_WGS = 256 * 4;          // events_audio_kernel's grid cap: four workgroups per CU (MI355X: 256 CUs)

struct AppendParams {
    const int16_t* src;           // [S][k][1280] the call's 16 kHz samples as the front end consumed them; nullptr = zero the streams
    int16_t* ring;                // [S][ring_chunks][1280]
    uint32_t* counter;            // [S]
    const uint8_t* stream_on;     // masked call: [S] 1 = the stream took part; nullptr = all did
    const int* ids;               // [n] the streams of the launch (a masked step's participants, a reset's list); nullptr = stream w
    int n;                        // waves with a stream: the list's length, or S
    int S;
    uint32_t k, ring_chunks;
};

// one 16-byte piece of the source: a vector load where the call's base is aligned, eight 2-byte loads where it is not
template <bool ALIGNED>
__device__ __forceinline__ uint4 load_piece(const int16_t* p) {
    if (ALIGNED) return *reinterpret_cast<const uint4*>(p);
    const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
    uint4 v;
    v.x = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
    v.y = (uint32_t)q[2] | ((uint32_t)q[3] << 16);
    v.z = (uint32_t)q[4] | ((uint32_t)q[5] << 16);
    v.w = (uint32_t)q[6] | ((uint32_t)q[7] << 16);
    return v;
}

template <bool ALIGNED>
__global__ __launch_bounds__(AU_WG) void audio_append_kernel(AppendParams p) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (AU_WG / 64) + (threadIdx.x >> 6);
    if (w >= p.n) return;
    const int s = p.ids ? p.ids[w] : w;
    if ((unsigned)s >= (unsigned)p.S) return;
    if (p.stream_on && !p.stream_on[s]) return;
    uint4* ring4 = reinterpret_cast<uint4*>(p.ring) + (size_t)s * p.ring_chunks * kChunkQuads;
    if (!p.src) {                                                // oww_reset: the ring and the counter read zero
        const int n_q = (int)p.ring_chunks * kChunkQuads;
        for (int i = lane; i < n_q; i += 64) ring4[i] = make_uint4(0u, 0u, 0u, 0u);
        if (lane == 0) p.counter[s] = 0u;
        return;
    }
    const uint32_t cnt = p.counter[s];                           // every lane, before any store of this wave
    const uint32_t c0 = first_kept(p.k, p.ring_chunks);
    const int n_q = (int)(p.k - c0) * kChunkQuads;               // <= ring_chunks * 160
    const int16_t* src = p.src + (size_t)s * p.k * OWW_CHUNK + (size_t)c0 * OWW_CHUNK;
    // piece i of the kept chunks: chunk c0 + i / 160 of the call, piece i % 160 of it
    auto dst = [&](int i) {
        const int c = i / kChunkQuads, e = i - c * kChunkQuads;
        return ring4 + (size_t)append_slot(cnt, c0 + (uint32_t)c, p.ring_chunks) * kChunkQuads + e;
    };
    // four pieces per lane and round, every load of a round ahead of its stores -- a one-chunk call (160 pieces: 64 + 64 + 32) is
    // one round with three loads in flight, not three dependent load-store pairs
    for (int i = lane; i < n_q; i += 4 * 64) {
        const bool h1 = i + 64 < n_q, h2 = i + 128 < n_q, h3 = i + 192 < n_q;
        uint4 v1 = make_uint4(0u, 0u, 0u, 0u), v2 = v1, v3 = v1;
        const uint4 v0 = load_piece<ALIGNED>(src + (size_t)i * 8);
        if (h1) v1 = load_piece<ALIGNED>(src + (size_t)(i + 64) * 8);
        if (h2) v2 = load_piece<ALIGNED>(src + (size_t)(i + 128) * 8);
        if (h3) v3 = load_piece<ALIGNED>(src + (size_t)(i + 192) * 8);
        *dst(i) = v0;
        if (h1) *dst(i + 64) = v1;
        if (h2) *dst(i + 128) = v2;
        if (h3) *dst(i + 192) = v3;
    }
    if (lane == 0) p.counter[s] = cnt + p.k;
}

struct GatherParams {
    const int16_t* ring;          // [S][ring_chunks][1280]
    const uint32_t* counter;      // [S]
    const int* ids;               // [n] listed streams (duplicates and any order)
    int16_t* out;                 // [n][n_chunks][1280], 16-byte aligned
    uint32_t* counts;             // [n] the listed streams' counters
    int S;
    uint32_t n_chunks, ring_chunks;
};

// one chunk, ring -> dst, or zeros: the wave's three pieces per lane (160 = 2 x 64 + 32) with the loads ahead of the stores
__device__ __forceinline__ void copy_chunk(const uint4* from /* nullptr = zeros */, uint4* to, int lane) {
    uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0, v2 = v0;
    const bool tail = lane + 128 < kChunkQuads;
    if (from) {
        v0 = from[lane]; v1 = from[lane + 64];
        if (tail) v2 = from[lane + 128];
    }
    to[lane] = v0; to[lane + 64] = v1;
    if (tail) to[lane + 128] = v2;
}

// grid (n, n_chunks), 64 threads: chunk blockIdx.y (0 = the oldest returned) of listed stream blockIdx.x
__global__ __launch_bounds__(64) void audio_gather_kernel(GatherParams p) {
    const int lane = threadIdx.x;
    const int s = p.ids[blockIdx.x];
    const uint32_t j = blockIdx.y;
    uint4* to = reinterpret_cast<uint4*>(p.out) + ((size_t)blockIdx.x * p.n_chunks + j) * kChunkQuads;
    const bool known = (unsigned)s < (unsigned)p.S;              // (the host checked the list: a bound, not a case)
    const uint32_t cnt = known ? p.counter[s] : 0u;
    uint32_t slot;
    const bool have = read_slot(cnt, p.n_chunks - 1u - j, p.ring_chunks, &slot);
    const uint4* from = have ? reinterpret_cast<const uint4*>(p.ring) + ((size_t)s * p.ring_chunks + slot) * kChunkQuads : nullptr;
    copy_chunk(from, to, lane);
    if (j == 0 && lane == 0) p.counts[blockIdx.x] = cnt;
}

struct EventsAudioParams {
    const int* count;             // {n_stored, n_total} of the call (events_write_kernel)
    const oww_event* rec;         // [capacity] records: rec[i].stream
    const int16_t* ring;
    const uint32_t* counter;
    int16_t* snap;                // [capacity + 1][event_chunks][1280]; snapshot i belongs to record i; the spare one is never written
    int S, capacity;
    uint32_t event_chunks, ring_chunks;
};

// grid min(AU_EVENT_WGS, what the capacity can need), 256 threads: wave = one chunk copy, grid stride over n_stored x event_chunks
__global__ __launch_bounds__(AU_WG) void events_audio_kernel(EventsAudioParams p) {
    const int lane = threadIdx.x & 63;
    int n_stored = p.count[0];
    n_stored = n_stored < 0 ? 0 : (n_stored < p.capacity ? n_stored : p.capacity);
    const long long n_items = (long long)n_stored * p.event_chunks;
    const long long step = (long long)gridDim.x * (AU_WG / 64);
    for (long long it = (long long)blockIdx.x * (AU_WG / 64) + (threadIdx.x >> 6); it < n_items; it += step) {
        const int rank = (int)(it / p.event_chunks);
        const uint32_t j = (uint32_t)(it - (long long)rank * p.event_chunks);
        const int s = p.rec[rank].stream;
        const bool known = (unsigned)s < (unsigned)p.S;
        const uint32_t cnt = known ? p.counter[s] : 0u;
        uint32_t slot;
        const bool have = read_slot(cnt, p.event_chunks - 1u - j, p.ring_chunks, &slot);
        const uint4* from = have ? reinterpret_cast<const uint4*>(p.ring) + ((size_t)s * p.ring_chunks + slot) * kChunkQuads : nullptr;
        copy_chunk(from, reinterpret_cast<uint4*>(p.snap) + (size_t)it * kChunkQuads, lane);
    }
}

}  // namespace owa
