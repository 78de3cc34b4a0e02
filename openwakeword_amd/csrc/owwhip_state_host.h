// owwhip_state_host.h -- what the host computes for stream state records (include/owwhip.h: oww_state_info / oww_state_export /
// oww_state_import / oww_move_streams; kernels and the record's description in owwhip_state.h): the record's constants and section
// table, the offsets of a list of sections, the configuration fingerprint, the group-block lists of one call and the refusals of ids
// and record headers.  Host only and free of HIP: owwhip.hip includes it for the library (state_layout: which buffers, the device copy
// of the table), owwhip_state.h for the constants and the table entry, tests/planners_check.cpp includes it alone under
// AddressSanitizer / UBSan.
#pragma once
#include "owwhip_pack.h"

namespace ows {

using owp::fail;

constexpr uint32_t kMagic = 0x5354574fu;          // "OWTS"
constexpr uint32_t kLayoutVersion = 1u;
constexpr int kHeaderWords = 8;

struct FlatSection {
    uint32_t* live;        // first stream's first word
    uint32_t stride;       // words per stream on the live side
    uint32_t len;          // words the stream owns
    uint32_t off;          // word offset in the record (a multiple of 4)
    uint32_t vec;          // 1 = the live side takes 16-byte accesses (stride and len multiples of 4)
};
// an array kept in blocks of spg streams, ppr positions of every run of 16 words per stream (il: position m * spg + p, else p * ppr + m)
struct GroupSection { float* live; int spg, ppr; bool il; uint32_t block_words, off; };

// ---- layout.  The record is [header | flat sections | group sections], in the order given; a section without a buffer or of no words
//      is dropped, every flat section is padded to 16 bytes.  Callers fill live / stride / len and live / spg / ppr / il / block_words;
//      off and vec are set here. ----
struct Layout { uint32_t flat_quads = 0, record_words = 0; };        // header + flat sections in 16-byte quads; the whole record in words
inline int layout(std::vector<FlatSection>& flat, std::vector<GroupSection>& group, Layout& L) {
    uint32_t off = kHeaderWords;
    flat.erase(std::remove_if(flat.begin(), flat.end(), [](const FlatSection& f) { return !f.live || f.len == 0; }), flat.end());
    for (FlatSection& f : flat) {
        f.off = off; f.vec = (uint32_t)(f.stride % 4 == 0 && f.len % 4 == 0);
        off += (f.len + 3) / 4 * 4;
    }
    L.flat_quads = off / 4;
    for (GroupSection& g : group) {
        const int R = g.ppr >= 4 ? 1 : 4 / std::max(g.ppr, 1);
        if (g.block_words % (16 * R) || (g.ppr != 1 && g.ppr != 2 && g.ppr != 4 && g.ppr != 8) || g.spg * g.ppr > 16)
            return fail(OWW_ESTATE, "state records: a group block of %u words, %d streams and %d positions per stream is not a layout the record kernels know", g.block_words, g.spg, g.ppr);
        g.off = off;
        off += g.block_words / 16 * g.ppr;
    }
    L.record_words = off;
    return 0;
}

// ---- fingerprint: what a record's bits depend on -- family, layouts, ring sizes, calibration scales and weights (the ingest and audio
//      configurations are mixed in behind it: owi::fingerprint, owa::fingerprint) ----
struct Blob { const void* p; size_t bytes; };
struct HeadPrint { int32_t hdr[6]; Blob weights; };       // kind, T, hidden, n_out, has_layernorm, n_blocks
inline uint64_t fingerprint(int use_mfma, bool il, const int* state_len, int n_state, int TR, int NL, int K, bool vad, const int* hx_e /*[20], or nullptr*/,
                            int hx_efeat, Blob mel, Blob emb, const std::vector<HeadPrint>& heads, Blob vad_net) {
    std::vector<int32_t> v = {(int32_t)kLayoutVersion, use_mfma, il ? 1 : 0};
    v.insert(v.end(), state_len, state_len + n_state);
    v.insert(v.end(), {TR, NL, K, vad ? 1 : 0});
    for (int l = 0; l < 20; ++l) v.push_back(hx_e ? hx_e[l] : 0);
    v.push_back(hx_e ? hx_efeat : 0);
    uint64_t fp = owp::fp_mix(1469598103934665603ull, v.data(), v.size() * sizeof(int32_t));
    fp = owp::fp_mix(fp, mel.p, mel.bytes);
    fp = owp::fp_mix(fp, emb.p, emb.bytes);
    for (const HeadPrint& h : heads) {
        fp = owp::fp_mix(fp, h.hdr, sizeof h.hdr);
        fp = owp::fp_mix(fp, h.weights.p, h.weights.bytes);
    }
    return owp::fp_mix(fp, vad_net.p, vad_net.bytes);
}

// ---- One list of streams as the record kernels want it: the ids in record order, and per group size (2, 4, 8, 16 streams) in use the
//      touched group blocks [group | record index of every place, -1 = not listed] -- found by one sort of the list, so that a block
//      whose streams are all listed is served by one workgroup per array as full rows.  Offsets are into the int buffer the lists are
//      uploaded in; a size no section uses has no blocks. ----
constexpr int kStateLevels[4] = {2, 4, 8, 16};
struct StateList { int n = 0; size_t ids_at = 0; size_t items_at[4] = {}; int n_groups[4] = {}; };

inline void state_list_build(const bool used[4], const int32_t* ids, int n, std::vector<int>& buf, StateList& L) {
    L.n = n; L.ids_at = buf.size();
    buf.insert(buf.end(), ids, ids + n);
    std::vector<std::pair<int, int>> order(n);
    for (int i = 0; i < n; ++i) order[i] = {ids[i], i};
    std::sort(order.begin(), order.end());
    for (int lv = 0; lv < 4; ++lv) {
        const int G = kStateLevels[lv];
        L.items_at[lv] = buf.size(); L.n_groups[lv] = 0;
        if (!used[lv]) continue;
        size_t cur = 0; int cur_g = -1;
        for (const auto& e : order) {
            const int g = e.first / G, place = e.first % G;
            if (g != cur_g || buf[cur + 1 + place] >= 0) {            // a new block (or a stream listed twice: a block entry of its own)
                cur = buf.size(); cur_g = g;
                buf.push_back(g);
                buf.insert(buf.end(), G, -1);
                ++L.n_groups[lv];
            }
            buf[cur + 1 + place] = e.second;
        }
    }
}

// ---- refusals ----
// ids in [0, S); unique where asked
inline int state_check_ids(int S, const char* fn, const char* what, const int32_t* ids, int n, bool unique) {
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= S) return fail(OWW_EINVAL, "%s: %s stream id %d out of range (0..%d)", fn, what, ids[i], S - 1);
    if (unique && n > 1) {
        std::vector<int32_t> t(ids, ids + n);
        std::sort(t.begin(), t.end());
        const auto dup = std::adjacent_find(t.begin(), t.end());
        if (dup != t.end()) return fail(OWW_EINVAL, "%s: %s stream id %d is listed twice", fn, what, *dup);
    }
    return 0;
}
// the 32-byte headers of n records (host copy) against a handle of `record_words` words per record and fingerprint `fp`
inline int state_check_headers(uint32_t record_words, uint64_t fp_mine, const uint32_t* hdr /*[n][8]*/, int n) {
    const uint32_t rb = record_words * 4;
    for (int i = 0; i < n; ++i) {
        const uint32_t* q = hdr + (size_t)i * kHeaderWords;
        if (q[0] != kMagic) return fail(OWW_EINVAL, "oww_state_import: record %d does not start with a stream state header (magic %08x)", i, q[0]);
        if (q[1] != kLayoutVersion)
            return fail(OWW_EINVAL, "oww_state_import: record %d has record layout version %u, this library reads version %u", i, q[1], kLayoutVersion);
        const uint64_t fp = (uint64_t)q[4] | ((uint64_t)q[5] << 32);
        if (q[2] != rb || fp != fp_mine)
            return fail(OWW_EINVAL, "oww_state_import: record %d comes from another configuration: the record carries fingerprint %016llx and %u bytes, "
                        "this handle has fingerprint %016llx and %u bytes (kernel family, ring sizes, bank slots, VAD, calibration scales or weights differ)",
                        i, (unsigned long long)fp, q[2], (unsigned long long)fp_mine, rb);
    }
    return 0;
}

}  // namespace ows
