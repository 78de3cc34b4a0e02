// mem_check -- the owning types of openwakeword_amd/csrc/owwhip_mem.h over a malloc-backed seam that counts live allocations, logs every
// call and can be told to fail the next allocation.  Stand-alone: no HIP, no GPU, not loaded into Python; tests/test_mem_host_cpu.py
// builds it with the host compiler under AddressSanitizer + UBSan (which see a double free, a leak or a use after release by
// themselves) and expects exit code 0 and "ok N checks" on stdout.  A failed check prints its line and makes the exit code 1.
#include "owwhip_mem.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

// ---- the seam over malloc ----
static std::set<void*> g_live;                     // every block, event and stream that is allocated and not yet released
static std::vector<std::string> g_log;             // "dev+ BYTES", "dev-", "pin+ BYTES FLAGS", "pin-", "ev+ FLAGS", "ev-", "st+ FLAGS", "st-"
static bool g_fail_next = false;
static int g_bad_release = 0;                      // releases of something that was not live (a double free)
static int g_last_line = 0;

static int take(void** p, size_t bytes, const std::string& what) {
    if (g_fail_next) { g_fail_next = false; g_log.push_back(what + " FAILED"); *p = (void*)0x10; return 2; }    // (a junk pointer nobody may keep)
    *p = malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    g_log.push_back(what);
    return 0;
}
static int give(void* p, const std::string& what) {
    if (!g_live.erase(p)) { ++g_bad_release; return 1; }
    free(p);
    g_log.push_back(what);
    return 0;
}
namespace owm {
int dev_alloc_raw(void** p, size_t bytes, int line) { g_last_line = line; return take(p, bytes, "dev+ " + std::to_string(bytes)); }
int dev_free_raw(void* p) { return give(p, "dev-"); }
int pinned_alloc_raw(void** p, size_t bytes, unsigned flags) { return take(p, bytes, "pin+ " + std::to_string(bytes) + " " + std::to_string(flags)); }
int pinned_free_raw(void* p) { return give(p, "pin-"); }
int event_create_raw(ihipEvent_t** e, unsigned flags) { return take((void**)e, 8, "ev+ " + std::to_string(flags)); }
int event_destroy_raw(ihipEvent_t* e) { return give(e, "ev-"); }
int stream_create_raw(ihipStream_t** s, unsigned flags) { return take((void**)s, 8, "st+ " + std::to_string(flags)); }
int stream_destroy_raw(ihipStream_t* s) { return give(s, "st-"); }
}  // namespace owm

using owm::DevBuf;
using owm::PinnedBuf;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_failed; printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)
// nothing live, nothing released twice; the log starts afresh
#define SCOPE_END() do { CHECK(g_live.empty()); CHECK(g_bad_release == 0); g_log.clear(); } while (0)
static bool log_is(std::initializer_list<const char*> want) {
    std::vector<std::string> w(want.begin(), want.end());
    return g_log == w;
}

// shaped like oww_ctx::IngestSlot / BankHead: several owners side by side, moved as a whole
struct Slot {
    DevBuf<short> d_pcm; DevBuf<float> d_scores; PinnedBuf<float> h_scores; PinnedBuf<unsigned char> h_on;
    owm::Event up, done, down;
    bool busy = false;
    bool fill(size_t n) {
        return !d_pcm.alloc(n) && !d_scores.alloc(n) && !h_scores.alloc(n, 0) && !h_on.alloc(n, 0) && !up.create(2) && !done.create(2) && !down.create(2);
    }
};

int main() {
    {   // alloc, conversion, capacity, release at scope exit; the call site's line reaches the seam
        DevBuf<float> b;
        CHECK(b.get() == nullptr && b.capacity() == 0 && !b);
        CHECK(b.alloc(10) == 0); const int line = __LINE__;
        CHECK(g_last_line == line);
        float* p = b;
        CHECK(p != nullptr && p == b.get() && b.capacity() == 10 && b + 3 == p + 3);
        CHECK(log_is({"dev+ 40"}) && g_live.size() == 1);
    }
    CHECK(log_is({"dev+ 40", "dev-"}));
    SCOPE_END();
    {   // reserve: nothing when it fits; growth frees once, then allocates once, exactly n
        DevBuf<int> b;
        CHECK(b.reserve(8) == 0 && b.capacity() == 8);
        int* p = b;
        g_log.clear();
        CHECK(b.reserve(8) == 0 && b.reserve(3) == 0 && b.reserve(0) == 0);
        CHECK(g_log.empty() && b.get() == p && b.capacity() == 8);
        CHECK(b.reserve(9) == 0);
        CHECK(log_is({"dev-", "dev+ 36"}) && b.capacity() == 9 && g_live.size() == 1);
        CHECK(b.alloc(2) == 0 && b.capacity() == 2);                      // alloc on a full buffer: the old block goes first
        CHECK(log_is({"dev-", "dev+ 36", "dev-", "dev+ 8"}) && g_live.size() == 1);
    }
    SCOPE_END();
    {   // a failed alloc / reserve: error returned, buffer empty (the old block is gone, as in every longhand copy), the next one succeeds
        DevBuf<float> b;
        g_fail_next = true;
        CHECK(b.alloc(4) == 2 && b.get() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(4) == 0 && b.capacity() == 4);
        g_fail_next = true;
        CHECK(b.reserve(5) == 2 && b.get() == nullptr && b.capacity() == 0 && g_live.empty());
        CHECK(b.reserve(5) == 0 && b.get() != nullptr && b.capacity() == 5);
        PinnedBuf<int> q;
        g_fail_next = true;
        CHECK(q.alloc(4, 0) == 2 && q.get() == nullptr && q.capacity() == 0);
        CHECK(q.reserve(4, 0) == 0 && q.capacity() == 4);
        owm::Event e;
        g_fail_next = true;
        CHECK(e.create(0) == 2 && e.get() == nullptr);
        CHECK(e.create(0) == 0 && e.get() != nullptr);
    }
    SCOPE_END();
    {   // 0 elements: one element, as max(n, 1)
        DevBuf<double> b;
        CHECK(b.alloc(0) == 0 && b.get() != nullptr && b.capacity() == 1 && log_is({"dev+ 8"}));
        PinnedBuf<short> q;
        CHECK(q.reserve(0, 0) == 0 && q.get() == nullptr);                // (nothing asked of an empty buffer: nothing done)
        CHECK(q.alloc(0, 0) == 0 && q.get() != nullptr && q.capacity() == 1);
    }
    SCOPE_END();
    {   // reset twice; reset of an empty buffer
        DevBuf<char> b, never;
        CHECK(b.alloc(3) == 0);
        b.reset(); b.reset(); never.reset();
        CHECK(b.get() == nullptr && b.capacity() == 0 && log_is({"dev+ 3", "dev-"}));
        owm::Stream s;
        CHECK(s.create(1) == 0);
        s.reset(); s.reset();
    }
    SCOPE_END();
    {   // move construction and move assignment: the source is empty, the destination's old block is released exactly once
        DevBuf<int> a, b;
        CHECK(a.alloc(4) == 0 && b.alloc(6) == 0);
        int* pa = a;
        DevBuf<int> c(std::move(a));
        CHECK(a.get() == nullptr && a.capacity() == 0 && c.get() == pa && c.capacity() == 4 && g_live.size() == 2);
        g_log.clear();
        b = std::move(c);
        CHECK(log_is({"dev-"}) && c.get() == nullptr && c.capacity() == 0 && b.get() == pa && b.capacity() == 4 && g_live.size() == 1);
        DevBuf<int>& self = b;
        b = std::move(self);                                              // onto itself: kept
        CHECK(b.get() == pa && b.capacity() == 4 && g_live.size() == 1);
        PinnedBuf<float> p, q;
        CHECK(p.alloc(2, 0) == 0 && q.alloc(2, 0) == 0);
        q = std::move(p);
        CHECK(p.get() == nullptr && g_live.size() == 2);
        owm::Event e, f;
        CHECK(e.create(2) == 0 && f.create(2) == 0);
        f = std::move(e);
        CHECK(e.get() == nullptr && f.get() != nullptr && g_live.size() == 3);
    }
    SCOPE_END();
    {   // PinnedBuf hands its flags on (2: a mapped allocation such as the range word's)
        PinnedBuf<int> r;
        CHECK(r.alloc(16, 2) == 0 && r.capacity() == 16);
        r[0] = 0; r[1] = -1;
        CHECK(r.reserve(17, 0) == 0);
        CHECK(log_is({"pin+ 64 2", "pin-", "pin+ 68 0"}));
    }
    SCOPE_END();
    {   // a borrowed stream is never destroyed; an owned one is, once; create on a borrowed one forgets it
        int dummy = 0;
        ihipStream_t* callers = reinterpret_cast<ihipStream_t*>(&dummy);
        {
            owm::Stream s;
            s.borrow(callers);
            CHECK(s.get() == callers);
            owm::Stream t(std::move(s));
            CHECK(s.get() == nullptr && t.get() == callers);
        }
        CHECK(g_log.empty());
        {
            owm::Stream s;
            s.borrow(callers);
            CHECK(s.create(1) == 0 && s.get() != callers);
        }
        CHECK(log_is({"st+ 1", "st-"}));
    }
    SCOPE_END();
    {   // a struct of owners in an array and in a vector, through reallocation and erase: everything released exactly once
        Slot pair[2];
        CHECK(pair[0].fill(5) && pair[1].fill(7));
        CHECK(g_live.size() == 14);
        std::vector<Slot> v;
        for (int i = 0; i < 9; ++i) {                                     // (grows through several reallocations)
            v.emplace_back();
            CHECK(v.back().fill(3 + i));
        }
        CHECK(g_live.size() == 14 + 9 * 7);
        v[4] = Slot{};                                                    // as oww_bank_remove empties a bank entry
        CHECK(g_live.size() == 14 + 8 * 7 && v[4].d_pcm.get() == nullptr);
        v.erase(v.begin() + 1);
        CHECK(g_live.size() == 14 + 7 * 7);
        v.resize(3);
        CHECK(g_live.size() == 14 + 3 * 7);
        v.clear(); v.resize(4);                                           // as alloc_bank sizes the bank
        CHECK(g_live.size() == 14 && v[3].d_scores.capacity() == 0);
        CHECK(v[0].d_pcm.alloc(2) == 0);
        g_fail_next = true;
        CHECK(v[0].d_scores.alloc(2) == 2 && g_live.size() == 15);        // a half-built slot releases what it got
    }
    SCOPE_END();
    if (g_failed) { printf("%d of %d checks failed\n", g_failed, g_checks); return 1; }
    printf("ok %d checks\n", g_checks);
    return 0;
}
