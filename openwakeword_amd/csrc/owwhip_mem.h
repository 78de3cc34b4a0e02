// owwhip_mem.h -- who owns what the host layer allocates: device buffers, page-locked host buffers, events and streams as move-only
// members and locals whose destructors release them.  Host only and free of HIP, like owwhip_pack.h: the runtime is reached through
// the few plain functions declared below, which owwhip.hip defines over HIP (its guard allocator included) and a plain host program
// over malloc (tests/mem_check.cpp runs every type below under AddressSanitizer / UBSan).  Error codes are the runtime's, 0 = success.
#pragma once
#include <cstddef>

struct ihipEvent_t;          // (the runtime's own names behind hipEvent_t / hipStream_t: opaque here)
struct ihipStream_t;

namespace owm {

// ---- the seam ----
int dev_alloc_raw(void** p, size_t bytes, int line);          // line: the call site the guard allocator prints
int dev_free_raw(void* p);
int pinned_alloc_raw(void** p, size_t bytes, unsigned flags);
int pinned_free_raw(void* p);
int event_create_raw(ihipEvent_t** e, unsigned flags);
int event_destroy_raw(ihipEvent_t* e);
int stream_create_raw(ihipStream_t** s, unsigned flags);
int stream_destroy_raw(ihipStream_t* s);

// One device allocation and its capacity in elements.  Converts to T*, so launch sites and pointer arithmetic read as with a raw
// pointer.  A request for 0 elements allocates one.
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() { if (p_) (void)dev_free_raw(p_); p_ = nullptr; cap_ = 0; }
    // releases what it holds, then allocates exactly max(n, 1) elements; on failure the buffer is empty
    int alloc(size_t n, int line = __builtin_LINE()) {
        reset();
        if (n == 0) n = 1;
        void* q = nullptr;
        if (const int e = dev_alloc_raw(&q, n * sizeof(T), line)) return e;
        p_ = static_cast<T*>(q); cap_ = n;
        return 0;
    }
    // nothing when n elements fit (every hot-path call); otherwise alloc(n): the contents are NOT kept
    int reserve(size_t n, int line = __builtin_LINE()) { return n <= cap_ ? 0 : alloc(n, line); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
};

// The same for page-locked host memory; flags: the runtime's hipHostMalloc* word.
template <class T>
class PinnedBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~PinnedBuf() { reset(); }
    void reset() { if (p_) (void)pinned_free_raw(p_); p_ = nullptr; cap_ = 0; }
    int alloc(size_t n, unsigned flags) {
        reset();
        if (n == 0) n = 1;
        void* q = nullptr;
        if (const int e = pinned_alloc_raw(&q, n * sizeof(T), flags)) return e;
        p_ = static_cast<T*>(q); cap_ = n;
        return 0;
    }
    int reserve(size_t n, unsigned flags) { return n <= cap_ ? 0 : alloc(n, flags); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
};

// An event or a stream (H: the runtime's handle, a pointer).  borrow(): somebody else's handle, used and never destroyed.
template <class H, int (*Create)(H*, unsigned), int (*Destroy)(H)>
class Owned {
    H h_ = nullptr;
    bool own_ = false;
public:
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h_(o.h_), own_(o.own_) { o.h_ = nullptr; o.own_ = false; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; own_ = o.own_; o.h_ = nullptr; o.own_ = false; }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() { if (h_ && own_) (void)Destroy(h_); h_ = nullptr; own_ = false; }
    int create(unsigned flags) {
        reset();
        if (const int e = Create(&h_, flags)) { h_ = nullptr; return e; }
        own_ = true;
        return 0;
    }
    void borrow(H h) { reset(); h_ = h; }
    operator H() const { return h_; }
    H get() const { return h_; }
};
using Event = Owned<ihipEvent_t*, event_create_raw, event_destroy_raw>;
using Stream = Owned<ihipStream_t*, stream_create_raw, stream_destroy_raw>;

}  // namespace owm
