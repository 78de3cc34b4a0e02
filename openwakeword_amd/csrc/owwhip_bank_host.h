// owwhip_bank_host.h -- what the host computes for the head bank (include/owwhip.h: oww_bank_*, oww_subscribe): the routing table of
// heads_bank_kernel (owwhip_hx.h) -- entries, tiles, waves per tile, the tile range of each width class, the first-layer weight bytes
// one step streams -- and the refusals of oww_bank_add's header and of the ids of oww_subscribe / oww_bank_remove /
// oww_bank_set_postproc.  Host only and free of HIP: owwhip.hip includes it for the library (bank_route: plan, grow, two uploads),
// owwhip_hx.h for the tile record, tests/planners_check.cpp includes it alone under AddressSanitizer / UBSan.  A bank head is anything
// with the members {live, ht, w1_bytes} (and T where a function says so): the handle's own record, or a test's.
#pragma once
#include <cstdlib>

#include "owwhip_pack.h"

namespace owh {
struct BankTile { int head, off, n, pad; };          // entries [off, off + n) of the entry list, all of bank head `head`
static_assert(sizeof(BankTile) == 16, "BankTile is one 16-byte load of heads_bank_kernel");
}  // namespace owh

namespace owb {

using owh::BankTile;
using owp::fail;

// ---- routing.  Per width class (0: ht 4, <= 64 hidden units; 1: ht 8, <= 128), each subscribed head's entries (stream * K + slot,
//      ascending) cut into tiles of 32 wg entries; wg = 4 waves (128 entries, one weight stream per 128) when the class's mean group
//      holds >= 96 entries, else one wave (32).  Tiles largest first within a class (stable; `sorted` = false keeps head order: the
//      OWH_BANK_PER_HEAD build), class 1 behind class 0.  A live head without subscribers contributes nothing. ----
struct Route {
    std::vector<int> entries;
    std::vector<BankTile> tiles;
    int wg[2] = {1, 1}, tile0[2] = {}, ntiles[2] = {}, entries_n[2] = {};     // per class: tiles [tile0, tile0 + ntiles), wg waves each
    std::vector<std::pair<int, int>> head_tiles[2];     // [first tile, count] of every subscribed head, before the sort
    double wbytes = 0.0;                                // first-layer weight bytes one step streams over all tiles
};
// OWW_BANK_WG (A/B aid): 1 or 4 waves per tile in both classes; anything else = the rule's own
inline int wg_env() {
    const char* e = getenv("OWW_BANK_WG");
    const int v = e ? atoi(e) : 0;
    return v == 1 || v == 4 ? v : 0;
}
template <class Head>
Route route(const int* sub /*[S][K], -1 = empty*/, int S, int K, const Head* heads, int cap, int wg_forced = 0, bool sorted = true) {
    std::vector<std::vector<int>> lists(cap);
    for (int i = 0; i < S * K; ++i) if (sub[i] >= 0) lists[sub[i]].push_back(i);
    Route r;
    for (int c = 0; c < 2; ++c) {
        auto mine = [&](int b) { return heads[b].live && (heads[b].ht == 8) == (c == 1) && !lists[b].empty(); };
        long long n_ent = 0; int n_grp = 0;
        for (int b = 0; b < cap; ++b) if (mine(b)) { n_ent += (long long)lists[b].size(); ++n_grp; }
        const int wg = wg_forced ? wg_forced : n_grp > 0 && n_ent >= 96LL * n_grp ? 4 : 1;
        r.wg[c] = wg;
        r.tile0[c] = (int)r.tiles.size();
        r.entries_n[c] = (int)n_ent;
        for (int b = 0; b < cap; ++b) {
            if (!mine(b)) continue;
            const int base = (int)r.entries.size(), n = (int)lists[b].size(), nt = (n + 32 * wg - 1) / (32 * wg);
            r.entries.insert(r.entries.end(), lists[b].begin(), lists[b].end());
            r.head_tiles[c].push_back({(int)r.tiles.size(), nt});
            for (int o = 0; o < n; o += 32 * wg) r.tiles.push_back(BankTile{b, base + o, std::min(32 * wg, n - o), 0});
            r.wbytes += (double)nt * (double)heads[b].w1_bytes;
        }
        if (sorted) std::stable_sort(r.tiles.begin() + r.tile0[c], r.tiles.end(), [](const BankTile& a, const BankTile& b) { return a.n > b.n; });
        r.ntiles[c] = (int)r.tiles.size() - r.tile0[c];
    }
    return r;
}

// ---- refusals: nothing has moved when one of them speaks ----
// the 8-word header of oww_bank_add's blob (kind, T, hidden, n_out, has_layernorm, extra_blocks, ..) against a feature ring of TR rows
inline int add_header_check(const int32_t* hdr, int TR) {
    const int kind = hdr[0], T = hdr[1], H = hdr[2], O = hdr[3], has_ln = hdr[4], extra = hdr[5];
    if (kind == 1) return fail(OWW_EINVAL, "oww_bank_add: gated heads are not accepted in the bank (load them as fixed heads)");
    if (kind == 2) return fail(OWW_EINVAL, "oww_bank_add: multiclass heads are not accepted in the bank (load them as fixed heads)");
    if (kind == 3) return fail(OWW_EINVAL, "oww_bank_add: recurrent heads are not accepted in the bank (load them as fixed heads)");
    if (kind != 0) return fail(OWW_EINVAL, "oww_bank_add: unknown head kind %d", kind);
    if (O != 1) return fail(OWW_EINVAL, "oww_bank_add: a bank head has one sigmoid output (n_out = %d)", O);
    if (extra != 0) return fail(OWW_EINVAL, "oww_bank_add: a bank head has exactly one hidden block (extra_blocks = %d)", extra);
    if (H < 1 || H > 128) return fail(OWW_EINVAL, "oww_bank_add: hidden = %d (a bank head has 1..128 hidden units)", H);
    if (T < 1 || T > TR) return fail(OWW_EINVAL, "oww_bank_add: T = %d exceeds the handle's feature ring (%d rows)", T, TR);
    if (has_ln != 0 && has_ln != 1) return fail(OWW_EINVAL, "oww_bank_add: has_layernorm = %d", has_ln);
    return 0;
}
template <class Head>
bool is_head(int id, const Head* heads, int cap) { return id >= 0 && id < cap && heads[id].live; }
template <class Head>
int head_id_check(const char* fn, int id, const Head* heads, int cap) {
    return is_head(id, heads, cap) ? 0 : fail(OWW_EINVAL, "%s: %d is not a bank head", fn, id);
}
// oww_subscribe: n streams, K bank ids each (-1 = leave the slot empty)
template <class Head>
int subscribe_check(const int32_t* stream_ids, int n, const int32_t* bank_ids, int S, int K, const Head* heads, int cap) {
    for (int i = 0; i < n; ++i) {
        if (stream_ids[i] < 0 || stream_ids[i] >= S) return fail(OWW_EINVAL, "oww_subscribe: stream id %d out of range (0..%d)", stream_ids[i], S - 1);
        for (int k = 0; k < K; ++k) {
            const int b = bank_ids[(size_t)i * K + k];
            if (b != -1 && !is_head(b, heads, cap)) return fail(OWW_EINVAL, "oww_subscribe: %d is not a bank head (stream %d, slot %d)", b, stream_ids[i], k);
        }
    }
    return 0;
}

}  // namespace owb
