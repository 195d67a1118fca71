// owners.h — the only owners of HIP resources in the library: device arrays, pinned host words, events, the engine's stream and opened IPC mappings.
// Each is move-only and gives back what it holds in its destructor (which never throws): a new buffer needs no line in any destructor, and a
// constructor that throws half-way leaks nothing.  The runtime's create / free calls for these resources appear in this file only (tests/test_abi_host.py).
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"

namespace mhip {

// Device array.  reserve: grow-only, contents NOT preserved, nothing zeroed.  alloc / set / update: exactly m elements (no allocation for m = 0), the last two
// filled from the host.  n is the element count asked for.  A failed allocation leaves p == nullptr, n == 0.
// FLAGS != 0: hipExtMallocWithFlags with them (the fine-grained receive region of the ghost exchange).
template <class U, unsigned FLAGS = 0> struct DBuf {
    U* p = nullptr; size_t n = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete; DBuf& operator=(const DBuf&) = delete;
    DBuf(DBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DBuf& operator=(DBuf&& o) noexcept { if (this != &o) { release(); p = std::exchange(o.p, nullptr); n = std::exchange(o.n, 0); } return *this; }
    ~DBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    void reserve(size_t m) { if (m > n) fresh(m, std::max<size_t>(m, 1)); }
    void alloc(size_t m) { fresh(m, m); }
    void set(const U* h, size_t m) { alloc(m); fill(h); }
    void set(const std::vector<U>& h) { set(h.data(), h.size()); }
    void update(const std::vector<U>& h) { if (h.size() != n) alloc(h.size()); fill(h.data()); }      // same length: the allocation stays
  private:
    void fresh(size_t m, size_t count) {      // the one allocation path: m elements asked for, count allocated
        release();
        if (!count) return;
        void* q = nullptr;
        if (FLAGS) MHIP_HIP(hipExtMallocWithFlags(&q, count * sizeof(U), FLAGS)); else MHIP_HIP(hipMalloc(&q, count * sizeof(U)));
        p = static_cast<U*>(q); n = m;
    }
    void fill(const U* h) { if (n) MHIP_HIP(hipMemcpy(p, h, n * sizeof(U), hipMemcpyHostToDevice)); }
};
static_assert(!std::is_copy_constructible<DBuf<int>>::value && !std::is_copy_assignable<DBuf<int>>::value, "owners move, they are never copied");

// One handle of the runtime and the call that gives it back; the owners below add how theirs is made, and convert to the raw handle where it is used.
template <class H, hipError_t (*GIVE_BACK)(H)> struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete; Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); } return *this; }
    ~Owned() { reset(); }
    void reset() { if (h) (void)GIVE_BACK(h); h = nullptr; }
};

// pinned host words, made once (of the size first asked for) and kept
template <class U> struct Pinned : Owned<void*, hipHostFree> {
    void make(size_t count) { if (!h) MHIP_HIP(hipHostMalloc(&h, count * sizeof(U))); }
    operator U*() const { return static_cast<U*>(h); }
};

// an event, made once: timing by default, hipEventDisableTiming for the ones only waited for
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    void make(unsigned flags = hipEventDefault) { if (!h) MHIP_HIP(hipEventCreateWithFlags(&h, flags)); }
    operator hipEvent_t() const { return h; }
};

// another process's device allocation mapped into this one
struct IpcMapping : Owned<void*, hipIpcCloseMemHandle> {
    void open(const hipIpcMemHandle_t& handle) { reset(); MHIP_HIP(hipIpcOpenMemHandle(&h, handle, hipIpcMemLazyEnablePeerAccess)); }
};

// The stream a context works on: its own (destroyed with it, or when a caller's stream replaces it) or a caller's (used, never destroyed).
struct Stream {
    hipStream_t s = nullptr; bool own_stream = false;
    Stream() = default;
    Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    ~Stream() { use(nullptr); }
    void create(unsigned flags) { use(nullptr); MHIP_HIP(hipStreamCreateWithFlags(&s, flags)); own_stream = true; }
    void use(hipStream_t callers) { if (own_stream && s) (void)hipStreamDestroy(s); s = callers; own_stream = false; }
    operator hipStream_t() const { return s; }
};
static_assert(!std::is_copy_constructible<Pinned<int>>::value && !std::is_copy_constructible<Event>::value && !std::is_copy_constructible<IpcMapping>::value &&
              !std::is_copy_constructible<Stream>::value, "owners move, they are never copied");

}  // namespace mhip
