// audio_check.cpp -- the host arithmetic of the per-stream audio rings (openwakeword_amd/csrc/owwhip_audio_host.h) as a plain host
// program: the header alone, no HIP, built with -fsanitize=address,undefined by tests/test_audio_cpu.py.  It walks the index map the
// kernels use against a std::deque per ring length, the 64-bit sizes at the largest request the entries accept, and every refusal.
// Output: "name value" lines the test reads; a failed self-check prints to stderr and exits 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#include "owwhip_audio_host.h"

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "audio_check: " __VA_ARGS__); fprintf(stderr, " [%s]\n", #cond); ++g_bad; } } while (0)

// the ring as the kernels keep it (slot -> chunk id, 0 = never written) beside a deque of the last `ring` chunk ids
static long walk(uint32_t ring, const std::vector<uint32_t>& calls, int rounds) {
    std::vector<uint32_t> slots(ring, 0u);
    std::deque<uint32_t> want;
    uint32_t counter = 0, next_id = 1;
    long reads = 0;
    for (int r = 0; r < rounds; ++r)
        for (uint32_t k : calls) {
            const uint32_t c0 = owa::first_kept(k, ring);
            CHECK(k - c0 == (k < ring ? k : ring), "ring %u k %u keeps %u chunks", ring, k, k - c0);
            std::vector<char> written(ring, 0);
            for (uint32_t c = 0; c < k; ++c) {
                const uint32_t id = next_id + c;
                want.push_back(id);
                if (want.size() > ring) want.pop_front();
                if (c < c0) continue;
                const uint32_t slot = owa::append_slot(counter, c, ring);
                CHECK(slot < ring, "ring %u: slot %u", ring, slot);
                CHECK(!written[slot], "ring %u k %u: slot %u written twice in one call", ring, k, slot);   // (lanes of one wave never collide)
                written[slot] = 1;
                slots[slot] = id;
            }
            counter += k; next_id += k;
            for (uint32_t age = 0; age < ring; ++age) {
                uint32_t slot = 0xffffffffu;
                const bool have = owa::read_slot(counter, age, ring, &slot);
                CHECK(have == (age < want.size()), "ring %u counter %u age %u: have %d", ring, counter, age, (int)have);
                CHECK(slot < ring, "ring %u: read slot %u", ring, slot);
                if (have) CHECK(slots[slot] == want[want.size() - 1 - age], "ring %u counter %u age %u: chunk %u, want %u", ring, counter, age,
                                slots[slot], want[want.size() - 1 - age]);
                ++reads;
            }
        }
    return reads;
}

int main() {
    // ---- the index map: several wraps at ring_chunks 1, 5 and 125, calls below, equal to and above the ring
    for (uint32_t ring : {1u, 5u, 125u}) {
        std::vector<uint32_t> calls = {1, 3, 7, 1, 1, ring, 2, ring + 1, 1, 2 * ring + 3, ring > 1 ? ring - 1 : 1, 1};
        printf("walk_%u %ld\n", ring, walk(ring, calls, 6));
    }
    {   // a reset stream reads nothing; one chunk later exactly one
        uint32_t slot = 9;
        CHECK(!owa::read_slot(0, 0, 5, &slot) && slot == 0, "an empty ring has a newest chunk");
        CHECK(owa::read_slot(1, 0, 5, &slot) && slot == 0 && !owa::read_slot(1, 1, 5, &slot), "after one chunk");
    }
    // ---- sizes: 64-bit throughout
    printf("ring_42gb %" PRIu64 "\n", owa::ring_bytes(131072, 125));
    printf("ring_max %" PRIu64 "\n", owa::ring_bytes(1048576, 1024));
    printf("counter_max %" PRIu64 "\n", owa::counter_bytes(1048576));
    printf("snap_max %" PRIu64 "\n", owa::snapshot_bytes(1 << 20, 1024));
    printf("gather_max %" PRIu64 "\n", owa::gather_bytes(1048576, 1024));
    printf("record_125 %" PRIu64 " record_0 %" PRIu64 " words_1024 %u quads %d\n", owa::record_growth_bytes(125), owa::record_growth_bytes(0),
           owa::ring_words(1024), owa::kChunkQuads);
    // ---- the fingerprint: nothing without audio, ring_chunks otherwise
    const uint64_t f0 = 0x1234567890abcdefull;
    CHECK(owa::fingerprint(f0, 0) == f0, "a handle without audio must hash nothing");
    CHECK(owa::fingerprint(f0, 5) != f0 && owa::fingerprint(f0, 5) != owa::fingerprint(f0, 6), "ring_chunks must reach the fingerprint");
    // ---- every refusal, and what passes
    auto line = [](const char* name, int rc) { printf("%s rc=%d %s\n", name, rc, rc ? owp::g_err.c_str() : "-"); };
    line("cfg_ok", owa::configure_check(true, false, 125, 25));
    line("cfg_ok_edges", owa::configure_check(true, false, 1, 1) | owa::configure_check(true, false, 1024, 0) | owa::configure_check(true, false, 1024, 1024));
    line("cfg_null", owa::configure_check(false, false, 5, 0));
    line("cfg_committed", owa::configure_check(true, true, 5, 0));
    line("cfg_ring0", owa::configure_check(true, false, 0, 0));
    line("cfg_ring_neg", owa::configure_check(true, false, -3, 0));
    line("cfg_ring_big", owa::configure_check(true, false, 1025, 0));
    line("cfg_ev_neg", owa::configure_check(true, false, 5, -1));
    line("cfg_ev_big", owa::configure_check(true, false, 5, 6));
    line("commit_ok", owa::commit_check(0, 0) | owa::commit_check(3, 16));
    line("commit_no_events", owa::commit_check(3, 0));
    line("ready_ok", owa::ready_check("oww_get_audio", true, true, 5));
    line("ready_null", owa::ready_check("oww_get_audio", false, false, 0));
    line("ready_uncommitted", owa::ready_check("oww_get_audio", true, false, 5));
    line("ready_no_audio", owa::ready_check("oww_get_event_audio", true, true, 0));
    const int32_t ids[4] = {69, 0, 0, 33}, bad_hi[2] = {0, 70}, bad_lo[1] = {-1};
    alignas(16) int16_t buf[16];
    line("get_ok", owa::get_audio_check(70, 5, ids, 4, 5, buf, 1) | owa::get_audio_check(70, 5, ids, 4, 1, buf, 0) | owa::get_audio_check(70, 5, nullptr, 0, 1, nullptr, 0));
    line("get_chunks0", owa::get_audio_check(70, 5, ids, 4, 0, buf, 0));
    line("get_chunks_big", owa::get_audio_check(70, 5, ids, 4, 6, buf, 0));
    line("get_id_hi", owa::get_audio_check(70, 5, bad_hi, 2, 1, buf, 0));
    line("get_id_lo", owa::get_audio_check(70, 5, bad_lo, 1, 1, buf, 0));
    line("get_null_list", owa::get_audio_check(70, 5, nullptr, 2, 1, buf, 0));
    line("get_null_out", owa::get_audio_check(70, 5, ids, 4, 1, nullptr, 0));
    line("get_n_neg", owa::get_audio_check(70, 5, ids, -1, 1, buf, 0));
    line("get_unaligned", owa::get_audio_check(70, 5, ids, 4, 1, buf + 1, 1));
    line("get_unaligned_host", owa::get_audio_check(70, 5, ids, 4, 1, buf + 1, 0));
    line("ev_ok", owa::event_audio_check(3, 0, 4, 4, buf, 0) | owa::event_audio_check(3, 4, 0, 4, nullptr, 0));
    line("ev_none", owa::event_audio_check(0, 0, 0, 4, buf, 0));
    line("ev_beyond", owa::event_audio_check(3, 2, 3, 4, buf, 0));
    line("ev_huge", owa::event_audio_check(3, 0x7fffffff, 0x7fffffff, 4, buf, 0));
    line("ev_first_neg", owa::event_audio_check(3, -1, 1, 4, buf, 0));
    line("ev_null_out", owa::event_audio_check(3, 0, 1, 4, nullptr, 0));
    line("ev_unaligned", owa::event_audio_check(3, 0, 1, 4, buf + 1, 1));
    if (g_bad) { fprintf(stderr, "audio_check: %d check(s) failed\n", g_bad); return 1; }
    return 0;
}
