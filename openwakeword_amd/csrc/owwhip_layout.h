// owwhip_layout.h -- compile-time constants that BOTH the host-side weight packer (owwhip_pack.h) and a kernel header depend on: the
// network's geometry, the per-stream state lengths, and the build switches that change the operand order of a packed weight.  Each is
// defined here once; no HIP, so a plain host program can include it (tests/pack_check.cpp).
#pragma once
#include <stdint.h>
#include <cstddef>

// ---- build switches that change a packed layout (-D variant builds: _build.build(defines=...)); the kernels they select are
// described where they live in owwhip_hx.h
// REM2: a k-step that carries ONE full channel tile (48 = 32 + 16) uses its empty half for the f16 split itself -- weights (wh | wh),
// (wl | 0): two MFMAs instead of three (owh::split_dup; pack_hx(..., rem2) packs the weight blocks accordingly)
#ifndef OWH_REM2
#define OWH_REM2 1
#endif
// position order inside a 16-position tile of stages C, D, E: p = SPT * mel + stream instead of p = F * stream + mel (owh::tile_pos)
#ifndef OWH_INTERLEAVE
#define OWH_INTERLEAVE 1
#endif
#ifndef OWH_WPS_C
#define OWH_WPS_C 2            // waves per SIMD of stage C (with OWH_WPS_A, B, D, E in owwhip_hx.h); 2 leaves room for OWH_KMERGE_MEL2
#endif
// K-merged form of a 1x3 (mel) layer whose input has a half remainder tile (72 = 64 + 8 channels: stage C layer c, stage D layer a):
// the three taps' remainders share one k-step (owh::merge_mel_rems); the weights come in pack_hx_tm order
#ifndef OWH_KMERGE_MEL
#define OWH_KMERGE_MEL 1
#endif
// ... and of one whose remainder tile is full (48 = 32 + 16: 2 k-steps instead of 3), only where the register budget has the 8 more
// operand registers per tile: layer a of stage C
#ifndef OWH_KMERGE_MEL2
#define OWH_KMERGE_MEL2 1
#endif
// K-merged form of the 3x1 (time) layers of stages whose channel count is not a multiple of 32: the remainder tiles of the three taps
// packed together, pair index = tap * NPR + v (owh::TimeK; pack_hx_tm packs the weights in the same order)
#ifndef OWH_KMERGE
#define OWH_KMERGE 1
#endif
#ifndef OWH_KMERGE_B
#define OWH_KMERGE_B 0     // stage B too (48 = 32 + 16 channels: 2 merged k-steps per OUTPUT row cost 16 more registers than the 6 source
                           // rows' separate remainder k-steps -> spills at 3 waves per SIMD); stage C (72 = 64 + 8) always
#endif
#ifndef OWH_KMERGE_MEL2B
#define OWH_KMERGE_MEL2B 0     // layer c of stage B (48 -> 48) in the same form: see DESIGN.md 5.2 for the measurement
#endif

namespace owk {
constexpr int RNN_H = 64, RNN_TMAX = 64;     // recurrent heads (heads_rnn_kernel): hidden units per direction, feature rows at most
constexpr int HD_MAXNETS = 8;                // heads64_kernel: nets per fast group
}  // namespace owk

namespace owh {
constexpr float WSCALE = 256.0f;            // heads / VAD: weights are stored as f16 halves of 2^8 * w
constexpr bool kInterleave = OWH_INTERLEAVE != 0;
}  // namespace owh

namespace owv {
// encoder weight blocks of 1 KB in LDS: layer l = [oct][tap][ks][part]
constexpr int V_BLK1 = 1 * 3 * 4 * 2, V_BLK2 = 2 * 3 * 1 * 2, V_BLK3 = 2 * 3 * 1 * 2, V_BLK4 = 4 * 3 * 1 * 2;
constexpr int V_WFLOATS = (V_BLK1 + V_BLK2 + V_BLK3 + V_BLK4) * 256;
}  // namespace owv

namespace owp {

struct LayerDef { int kh, kw, cin, cout; };
inline constexpr LayerDef kLayers[20] = {
    {3, 3, 1, 24},
    {1, 3, 24, 24}, {3, 1, 24, 24},
    {1, 3, 24, 48}, {3, 1, 48, 48}, {1, 3, 48, 48}, {3, 1, 48, 48},
    {1, 3, 48, 72}, {3, 1, 72, 72}, {1, 3, 72, 72}, {3, 1, 72, 72},
    {1, 3, 72, 96}, {3, 1, 96, 96}, {1, 3, 96, 96}, {3, 1, 96, 96},
    {1, 3, 96, 96}, {3, 1, 96, 96}, {1, 3, 96, 96}, {3, 1, 96, 96},
    {3, 1, 96, 96},
};
// new rows x F x C of every layer's output per step (debug layout)
inline constexpr int kLayerOut[20][3] = {
    {8, 32, 24}, {8, 32, 24}, {8, 32, 24},
    {4, 16, 48}, {4, 16, 48}, {4, 16, 48}, {4, 16, 48},
    {4, 8, 72}, {4, 8, 72}, {4, 8, 72}, {4, 8, 72},
    {2, 4, 96}, {2, 4, 96}, {2, 4, 96}, {2, 4, 96},
    {2, 2, 96}, {2, 2, 96}, {2, 2, 96}, {2, 2, 96},
    {1, 1, 96},
};
constexpr int DBG_FLOATS = 3 * 6144 + 4 * 3072 + 4 * 2304 + 4 * 768 + 4 * 384 + 96;

constexpr int N_STATE = 11;
// per-stream floats of every state array: hist_mel, hist2, B:b,d  C:b,d  D:b,d  E:b,d  hist19
inline constexpr int kStateLenLds[N_STATE] = {64, 1536, 1536, 1536, 1152, 1152, 768, 768, 384, 384, 192};
// register-resident layout: channel tiles padded to 16 (24->32, 72->80), streams of one wave interleaved per block
inline constexpr int kStateLenRr[N_STATE] = {64, 2048, 1536, 1536, 1280, 1280, 768, 768, 384, 384, 384};
inline constexpr int kStateSpgRr[N_STATE] = {1, 1, 1, 1, 2, 2, 4, 4, 8, 8, 8};
inline constexpr int kStateFposRr[N_STATE] = {16, 16, 16, 16, 8, 8, 4, 4, 2, 2, 1};
// pooled activations handed from stage to stage, floats per stream: xA, xB, xC, xD
inline constexpr int kXLenLds[4] = {1536, 1536, 576, 384};
inline constexpr int kXLenRr[4] = {2048, 1536, 640, 384};

// blob of oww_load_vad (floats after the 8-int header): gain, hann[256], 4 x (w[3][cin][cout], b[cout]), 2 x (w[128][256], b[256]), wd[64], bd
inline constexpr int kVadEnc[4][2] = {{128, 16}, {16, 32}, {32, 32}, {32, 64}};
constexpr size_t vad_blob_floats() {
    size_t n = 1 + 256;
    for (auto& e : kVadEnc) n += (size_t)3 * e[0] * e[1] + e[1];
    n += 2 * ((size_t)128 * 256 + 256) + 64 + 1;
    return n;
}
// pack_hx of the four encoder layers, back to back, is the image owv::vad_front_kernel copies into LDS
constexpr int vad_enc_floats(int l) { return (kVadEnc[l][1] + 15) / 16 * 3 * ((kVadEnc[l][0] + 31) / 32) * 2 * 256; }
static_assert(vad_enc_floats(0) == owv::V_BLK1 * 256 && vad_enc_floats(1) == owv::V_BLK2 * 256 && vad_enc_floats(2) == owv::V_BLK3 * 256 &&
              vad_enc_floats(3) == owv::V_BLK4 * 256, "kVadEnc and the V_BLK* block counts describe the same encoder");

// Half channel tiles of the fp16-split family (24 = 16 + 8, 72 = 64 + 8 channels).  The MFMA D layout puts row 4j + e of a tile into
// register e of lane group j; with the natural order the 8 real channels of the last tile would sit in registers 0..3 of lane groups
// 0, 1 and no register would be all padding.  The f16-split kernels instead place them in registers 0, 1 of ALL four lane groups:
//     row 4j + e of the half tile  <->  channel 16 ct + 2j + e   (e < 2),   rows with e >= 2: padding
// so that registers 2, 3 of that tile are identically zero and their epilogue, operand split, loads and stores can be skipped.
// The same order is the K order of the layer that consumes the tile (operand halves q % 4 = e of lane group g = j), of the folded
// BatchNorm arrays and of the debug dump (owh::dump_tile_ht).
inline int hx_row_channel(int tile, int row, int C) {            // channel in row `row` (0..15) of channel tile `tile`, or -1
    const bool half = C % 16 == 8 && tile == (C + 15) / 16 - 1;
    if (!half) { const int c = tile * 16 + row; return c < C ? c : -1; }
    const int j = row >> 2, e = row & 3;
    return e < 2 ? tile * 16 + 2 * j + e : -1;
}

}  // namespace owp
