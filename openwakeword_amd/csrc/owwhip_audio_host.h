// owwhip_audio_host.h -- everything the host knows about the per-stream audio rings (include/owwhip.h: oww_audio_configure, oww_get_audio,
// oww_get_event_audio): the argument checks of every entry, the 64-bit buffer sizes, the index map of the ring (which slot a call's
// chunk lands in, which chunks of a long call are kept, which slot holds the chunk of a given age and when it reads as zero), and the
// audio part of the state fingerprint and of the record's section table.  Host only and free of HIP, like owwhip_ingest.h: owwhip.hip
// includes it for the library, tests/audio_check.cpp includes it alone under AddressSanitizer / UBSan.  The index map is marked for
// both sides where a HIP compiler reads this file, so that the kernels of owwhip_audio.h walk the very functions the host program tests.
#pragma once
#include <cstdint>

#include "owwhip.h"
#include "owwhip_pack.h"

#ifdef __HIPCC__
#define OWA_HD __host__ __device__ __forceinline__
#else
#define OWA_HD inline
#endif

namespace owa {

using owp::fail;

constexpr int kMaxRing = 1024;                        // ring_chunks: 1 .. 1024 (the reference's 10 s: 125)
constexpr int kChunkQuads = OWW_CHUNK * 2 / 16;       // 16-byte pieces of one chunk: 160
constexpr uint64_t kChunkBytes = (uint64_t)OWW_CHUNK * sizeof(int16_t);

// ---- the ring's index map.  A stream's counter counts the chunks it received since its reset; 32 bits of 80 ms chunks are 10.9 years,
//      and the map holds up to there (a ring length that does not divide 2^32 would skip slots at the wrap). ----

// chunk c of a call that found the counter at `counter` lands in this slot
OWA_HD uint32_t append_slot(uint32_t counter, uint32_t c, uint32_t ring_chunks) { return (counter + c) % ring_chunks; }

// a call of k chunks keeps its last min(k, ring_chunks): the first kept chunk of the call
OWA_HD uint32_t first_kept(uint32_t k, uint32_t ring_chunks) { return k > ring_chunks ? k - ring_chunks : 0u; }

// The chunk of age `age` (0 = the newest, age < ring_chunks) of a stream whose counter reads `counter`: false = the stream has not
// received it since its reset and it reads as zero; true = it sits in *slot.
OWA_HD bool read_slot(uint32_t counter, uint32_t age, uint32_t ring_chunks, uint32_t* slot) {
    if (age >= counter) { *slot = 0; return false; }
    *slot = (counter - 1u - age) % ring_chunks;
    return true;
}

// ---- sizes, in bytes, 64-bit throughout: 131,072 streams x 125 chunks x 2,560 B = 42 GB is a legitimate request ----
inline uint64_t ring_bytes(int64_t n_streams, int64_t ring_chunks) { return (uint64_t)n_streams * (uint64_t)ring_chunks * kChunkBytes; }
inline uint64_t counter_bytes(int64_t n_streams) { return (uint64_t)n_streams * sizeof(uint32_t); }
// snapshots of one event buffer set: capacity + 1 (the spare one the library never writes)
inline uint64_t snapshot_bytes(int64_t capacity, int64_t event_chunks) { return ((uint64_t)capacity + 1u) * (uint64_t)event_chunks * kChunkBytes; }
inline uint64_t gather_bytes(int64_t n, int64_t n_chunks) { return (uint64_t)n * (uint64_t)n_chunks * kChunkBytes; }

// ---- argument checks: nothing has moved when one of them refuses ----
inline int configure_check(bool have_handle, bool committed, int32_t ring_chunks, int32_t event_chunks) {
    if (!have_handle) return fail(OWW_EINVAL, "oww_audio_configure: null handle");
    if (committed) return fail(OWW_ESTATE, "oww_audio_configure: call before oww_commit");
    if (ring_chunks < 1 || ring_chunks > kMaxRing) return fail(OWW_EINVAL, "oww_audio_configure: ring_chunks = %d outside [1, %d]", ring_chunks, kMaxRing);
    if (event_chunks < 0 || event_chunks > ring_chunks)
        return fail(OWW_EINVAL, "oww_audio_configure: event_chunks = %d outside [0, ring_chunks = %d]", event_chunks, ring_chunks);
    return 0;
}

// oww_commit: snapshots per event need events
inline int commit_check(int32_t event_chunks, int32_t event_capacity) {
    if (event_chunks > 0 && event_capacity <= 0)
        return fail(OWW_EINVAL, "oww_audio_configure: event_chunks = %d needs events (oww_events_configure before oww_commit)", event_chunks);
    return 0;
}

// the three read entries on a handle that is not committed or keeps no audio
inline int ready_check(const char* fn, bool have_handle, bool committed, int32_t ring_chunks) {
    if (!have_handle) return fail(OWW_EINVAL, "%s: null handle", fn);
    if (!committed || ring_chunks <= 0) return fail(OWW_ESTATE, "%s: the handle keeps no audio (oww_audio_configure before oww_commit)", fn);
    return 0;
}

inline int get_audio_check(int32_t n_streams, int32_t ring_chunks, const int32_t* stream_ids, int32_t n, int32_t n_chunks, const void* out,
                           int out_on_device) {
    if (n < 0 || (n > 0 && (!stream_ids || !out))) return fail(OWW_EINVAL, "oww_get_audio: bad argument (n = %d, null list or buffer)", n);
    if (n_chunks < 1 || n_chunks > ring_chunks) return fail(OWW_EINVAL, "oww_get_audio: n_chunks = %d outside [1, ring_chunks = %d]", n_chunks, ring_chunks);
    for (int32_t i = 0; i < n; ++i)
        if (stream_ids[i] < 0 || stream_ids[i] >= n_streams)
            return fail(OWW_EINVAL, "oww_get_audio: stream id %d out of range (0..%d)", stream_ids[i], n_streams - 1);
    if (n > 0 && out_on_device && (reinterpret_cast<uintptr_t>(out) & 15)) return fail(OWW_EINVAL, "oww_get_audio: a device buffer must be 16-byte aligned");
    return 0;
}

// `stored`: records the call oww_get_events refers to stored
inline int event_audio_check(int32_t event_chunks, int32_t first, int32_t n, int32_t stored, const void* out, int out_on_device) {
    if (event_chunks == 0) return fail(OWW_EINVAL, "oww_get_event_audio: the handle keeps no audio snapshots (event_chunks = 0)");
    if (first < 0 || n < 0 || (int64_t)first + n > stored)
        return fail(OWW_EINVAL, "oww_get_event_audio: events [%d, %d + %d) of %d stored", first, first, n, stored);
    if (n > 0 && !out) return fail(OWW_EINVAL, "oww_get_event_audio: out is null");
    if (n > 0 && out_on_device && (reinterpret_cast<uintptr_t>(out) & 15)) return fail(OWW_EINVAL, "oww_get_event_audio: a device buffer must be 16-byte aligned");
    return 0;
}

// ---- state records: with audio the record gains two flat sections behind the existing ones, the ring as it lies ([ring_chunks][1280]
//      int16 = ring_words words, slot order: the counter that travels with it says where the newest chunk sits) and one 16-byte piece
//      with the counter.  The fingerprint covers ring_chunks; a handle without audio hashes nothing. ----
inline uint32_t ring_words(int32_t ring_chunks) { return (uint32_t)ring_chunks * (uint32_t)(OWW_CHUNK / 2); }
constexpr uint32_t kCounterWords = 1;
inline uint64_t record_growth_bytes(int32_t ring_chunks) { return ring_chunks > 0 ? (uint64_t)ring_words(ring_chunks) * 4u + 16u : 0u; }

inline uint64_t fingerprint(uint64_t fp, int32_t ring_chunks) {
    if (ring_chunks <= 0) return fp;
    const int32_t tag[2] = {-2, ring_chunks};           // (no ingest configuration hashes a leading -2)
    return owp::fp_mix(fp, tag, sizeof tag);
}

}  // namespace owa
