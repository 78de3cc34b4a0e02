// owwhip_dense_host.h -- everything the host knows about dense scoring (include/owwhip.h: oww_score_shape, oww_score_features,
// oww_score_clips): the window count and each head's row offset, the tiling of the sliding-window kernel (owwhip_dense.h), its LDS
// geometry and the largest T it takes, the slab arithmetic of the gather fallback, and the argument checks of the three entries.  Host
// only and free of HIP, like owwhip_audio_host.h: owwhip.hip includes it for the library, tests/dense_check.cpp includes it alone under
// AddressSanitizer / UBSan.  The two layout functions are marked for both sides where a HIP compiler reads this file, so that the kernel
// addresses its staged rows through the very functions the host program tests.
#pragma once
#include <cstdint>
#include <initializer_list>

#include "owwhip.h"
#include "owwhip_pack.h"

#ifdef __HIPCC__
#define OWD_HD __host__ __device__ __forceinline__
#else
#define OWD_HD inline
#endif

namespace owd {

using owp::fail;

// ---- windows.  Window w of a sequence ends at row w + t_max - 1; a head of window length T reads its own last T rows,
//      [w + t_max - T, w + t_max): what the heads of one live handle see at one instant. ----
inline int64_t n_win(int64_t n_rows, int64_t t_max) { return n_rows - t_max + 1; }           // <= 0: the sequence is too short
inline int64_t row_offset(int64_t t_max, int64_t T) { return t_max - T; }                    // first row of window 0 for a head of length T

// ---- the sliding-window kernel's tile: one workgroup of `waves` waves scores 32 x waves consecutive windows of one sequence (two
//      position tiles of 16 per wave, as heads_hx_kernel).  The first-layer weights stream L2 -> LDS once per TILE, and that stream is
//      what bounds the heads launches at full size (4.3 GB for 360,000 windows x 4 nets at 128 windows per workgroup), so the tile is
//      256 windows (8 waves) wherever its rows fit the LDS and 128 (4 waves) for the longer T. ----
constexpr int kWavesBig = 8, kWavesSmall = 4;
inline int64_t tile_windows(int waves) { return 32 * (int64_t)waves; }
inline int64_t tiles_per_seq(int64_t nw, int waves) { return (nw + tile_windows(waves) - 1) / tile_windows(waves); }
inline int64_t tile_rows(int64_t T, int waves) { return tile_windows(waves) + T - 1; }      // rows a tile stages

// ---- staged rows in LDS.  A row is 96 features = 12 units of 8; a unit is what one lane feeds one k-step: 8 hi halves (16 bytes) then
//      8 lo halves (16 bytes), 8 words.  The 16 positions of a tile read the same unit of 16 consecutive rows in one instruction, so
//      the row stride decides the banks: 96 words would put rows 2 apart on the same bank (96 * 2 = 3 * 64); with 100 words the 16 rows
//      start at 36 r mod 64 = {0, 36, 8, 44, 16, 52, 24, 60, 32, 4, 40, 12, 48, 20, 56, 28} -- sixteen distinct multiples of 4, so
//      their 16-byte reads cover the 64 banks exactly once.  (The hardware serves a 16-byte read in four groups of 16 lanes that
//      each mix eight positions of one unit with the other eight of the next unit, 8 words on: of a group's sixteen 4-bank slots two
//      are then hit twice, none more often -- four of a k-step's 20 or 36 LDS reads, against every one of them at a 96-word stride.) ----
constexpr int kRowWords = 100;
constexpr int kUnitWords = 8;
OWD_HD int unit_word(int row, int unit) { return row * kRowWords + unit * kUnitWords; }      // word offset of (row, unit); lo half at + 4
OWD_HD int kstep_unit(int ks, int j) { return (ks % 3) * 4 + j; }                            // k-step ks = (row ks / 3, features 32 (ks % 3) + 8 j ..)

// ---- passes.  A launch takes one or two nets of a fast group (a PASS): with two nets a k-step chunk is 16 KB, which leaves the LDS
//      to the rows of a 256-window tile and a ring of three slots at T = 16; the nets of a group beyond two go to further launches,
//      each streaming only its own nets' blocks of every chunk.  A gated pair (net i, role 0; net i + 1, role 1, same head) is never
//      split: the second net's score replaces the first's in the same lane.  out[k] = {first net, nets}; returns the pass count. ----
constexpr int kMaxPassNets = 2;
inline bool gated_pair(const int* role, const int* head, int n, int i) { return i + 1 < n && role[i + 1] == 1 && head[i + 1] == head[i]; }
inline int split_passes(const int* role, const int* head, int n, int (*out)[2]) {
    int k = 0;
    for (int i = 0; i < n;) {
        const int nn = (i + 1 < n && (gated_pair(role, head, n, i) || !gated_pair(role, head, n, i + 1))) ? 2 : 1;
        out[k][0] = i; out[k][1] = nn; ++k; i += nn;
    }
    return k;
}

// ---- LDS geometry of one launch: staged rows (dynamic) + the weight ring (static slots).  A k-step chunk of a pass is
//      n_nets x 4 hidden tiles x 2 parts x 1 KB.  A tile's workgroup is alone on its CU (its LDS leaves no room for a second one), so the
//      ring is as deep as fits, up to kMaxSlots: chunks in flight are what hides the L2 round trip. ----
constexpr int64_t kLdsBytes = 160 * 1024;
constexpr int kMinSlots = 2, kMaxSlots = 4;
inline int64_t chunk_bytes(int n_nets) { return (int64_t)n_nets * 4 * 2 * 1024; }
inline int64_t staged_bytes(int64_t T, int waves) { return tile_rows(T, waves) * kRowWords * 4; }
struct Geometry {
    int waves = 0, slots = 0;      // waves per workgroup and ring slots of the launch; 0 = the pass does not fit and takes the fallback
    int64_t rows = 0, staged = 0, ring = 0, total = 0;      // bytes (0 when it does not fit)
};
inline Geometry geometry(int n_nets, int64_t T) {
    Geometry g;
    if (n_nets < 1 || n_nets > kMaxPassNets || T < 1) return g;
    for (int waves : {kWavesBig, kWavesSmall}) {
        if (staged_bytes(T, waves) + chunk_bytes(n_nets) * kMinSlots > kLdsBytes) continue;
        g.waves = waves; g.rows = tile_rows(T, waves); g.staged = staged_bytes(T, waves);
        for (int s = kMaxSlots; s >= kMinSlots; --s)
            if (g.staged + chunk_bytes(n_nets) * s <= kLdsBytes) { g.slots = s; break; }
        g.ring = chunk_bytes(n_nets) * g.slots; g.total = g.staged + g.ring;
        return g;
    }
    return g;
}
// the largest T a tile of `waves` waves takes for a pass of n_nets nets: (32 waves + T - 1) x 400 + 2 x n_nets x 8 KB <= 160 KB
//   8 waves: 113 (one net), 72 (two);  4 waves: 241, 200 -- beyond the ABI's longest window (120), so every narrow group slides
inline int64_t t_limit(int n_nets, int waves) { return (kLdsBytes - chunk_bytes(n_nets) * kMinSlots) / (kRowWords * 4) - tile_windows(waves) + 1; }

// ---- the gather fallback: windows [n][T][96] materialised into a bounded slab, slab after slab ----
constexpr int64_t kSlabBytes = 256ll << 20;            // 256 MiB: 43,690 windows at T = 16, a heads launch of 342 workgroups
constexpr int64_t kWindowRowBytes = 96 * 4;
struct Slab { int64_t windows = 0, n_slabs = 0, bytes = 0; };          // windows per slab, slabs, bytes of one slab
inline Slab slab(int64_t total_windows, int64_t T, int64_t budget = kSlabBytes) {
    Slab s;
    if (total_windows < 1 || T < 1) return s;
    const int64_t per = T * kWindowRowBytes;
    s.windows = std::max<int64_t>(1, std::min<int64_t>(budget / per, total_windows));
    s.windows = std::min<int64_t>(s.windows, INT32_MAX);                // a slab is one heads launch: its positions are 32-bit
    s.n_slabs = (total_windows + s.windows - 1) / s.windows;
    s.bytes = s.windows * per;
    return s;
}

// ---- sizes, in bytes, 64-bit throughout ----
inline uint64_t feats_bytes(int64_t B, int64_t n_rows) { return (uint64_t)B * (uint64_t)n_rows * kWindowRowBytes; }
inline uint64_t out_bytes(int64_t B, int64_t nw, int64_t n_labels) { return (uint64_t)B * (uint64_t)nw * (uint64_t)n_labels * 4u; }
constexpr uint64_t kMaxBytes = 1ull << 40;             // no single buffer of a call is larger than 1 TiB
constexpr int64_t kMaxGrid = INT32_MAX;                // workgroups of one launch

// ---- argument checks: nothing has moved when one of them refuses.  t_max: the largest T over the handle's fixed heads (0 = none). ----
inline int ready_check(const char* fn, bool have_handle, bool committed, int n_heads) {
    if (!have_handle || !committed) return fail(OWW_ESTATE, "%s: handle not committed", fn);
    if (n_heads < 1) return fail(OWW_EINVAL, "%s: the handle has no fixed heads (bank heads are not scored densely)", fn);
    return 0;
}
inline int shape_check(const char* fn, int64_t n_rows, int64_t t_max) {
    if (n_rows < t_max) return fail(OWW_EINVAL, "%s: n_rows = %lld is less than one window (t_max = %lld)", fn, (long long)n_rows, (long long)t_max);
    return 0;
}
// a feature matrix of any entry, fixed heads or bank: one window at least, and aligned where it is the caller's device buffer
inline int rows_check(const char* fn, const void* feats, int feats_on_device, int64_t n_rows, int64_t t_max) {
    if (int rc = shape_check(fn, n_rows, t_max)) return rc;
    if (feats_on_device && (reinterpret_cast<uintptr_t>(feats) & 15)) return fail(OWW_EINVAL, "%s: device features must be 16-byte aligned", fn);
    return 0;
}
inline int features_check(const char* fn, const void* feats, int feats_on_device, int64_t B, int64_t n_rows, int64_t t_max, int64_t n_labels,
                          const void* out, int out_on_device) {
    if (!feats || !out || B < 1) return fail(OWW_EINVAL, "%s: bad argument (B = %lld, null features or output)", fn, (long long)B);
    if (int rc = rows_check(fn, feats, feats_on_device, n_rows, t_max)) return rc;
    (void)out_on_device;
    const int64_t nw = n_win(n_rows, t_max);
    const uint64_t fb = feats_bytes(B, n_rows), ob = out_bytes(B, nw, n_labels);
    if (fb > kMaxBytes || ob > kMaxBytes || (uint64_t)B * (uint64_t)n_rows > (uint64_t)INT64_MAX / 1024)
        return fail(OWW_ENOMEM, "%s: %llu bytes of features and %llu bytes of scores do not fit", fn, (unsigned long long)fb, (unsigned long long)ob);
    if (B * tiles_per_seq(nw, kWavesSmall) > kMaxGrid)
        return fail(OWW_ENOMEM, "%s: %lld sequences x %lld tiles exceed one launch (%llu bytes of scores); score in chunks", fn, (long long)B,
                    (long long)tiles_per_seq(nw, kWavesSmall), (unsigned long long)ob);
    return 0;
}
// oww_score_clips: n samples per clip -> n_out embedding rows, as oww_embed_clips (which repeats its own checks on the same numbers)
inline int64_t clip_rows(int64_t n) {
    if (n < 512) return 0;
    const int64_t F = (n - 512) / 160 + 1;
    return F < 76 ? 0 : (F - 76) / 8 + 1;
}
inline int clips_check(const char* fn, const void* pcm, int64_t B, int64_t n, int64_t n_streams, int64_t t_max, int64_t n_labels, const void* out) {
    if (!pcm || !out || B < 1 || B > n_streams) return fail(OWW_EINVAL, "%s: bad argument (B = %lld, need 1 <= B <= %lld)", fn, (long long)B, (long long)n_streams);
    const int64_t rows = clip_rows(n);
    if (rows < 1) return fail(OWW_EINVAL, "%s: %lld samples give no embedding (one needs 12,512)", fn, (long long)n);
    if (int rc = shape_check(fn, rows, t_max)) return rc;
    const uint64_t ob = out_bytes(B, n_win(rows, t_max), n_labels);
    if (feats_bytes(B, rows) > kMaxBytes || ob > kMaxBytes) return fail(OWW_ENOMEM, "%s: %llu bytes of scores do not fit", fn, (unsigned long long)ob);
    return 0;
}

}  // namespace owd
