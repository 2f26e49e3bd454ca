// sspp_own.h — the owning types of the host code's GPU resources (host only).
//
// Dev<T> a device buffer, Pinned<T> pinned host memory, Event a HIP event, Staging the pinned source
// of asynchronous copies with the event that guards it, Retired the device buffers a job replaced
// while launches may still read them.  None can be copied, all but Staging (a member that stays where
// it is) can be moved, and all free what they hold when they die; a
// failed allocation leaves its object empty and returns SSPP_E_NOMEM, every other HIP failure
// SSPP_E_HIP (hip_fail / HIPCHK).  g_live counts what is alive (sspp_debug_live_resources).
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <string>
#include <utility>
#include <vector>

#include "model.h"

namespace sspo {

// SSPP_OK for hipSuccess, else the thread's error set to "what: <HIP's message>"
inline int hip_fail(hipError_t e, const char* what) {
    if (e == hipSuccess) return SSPP_OK;
    return sspp::set_error(SSPP_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(x)                                             \
    do {                                                      \
        if (int rc_ = sspo::hip_fail((x), #x)) return rc_;    \
    } while (0)

inline int nomem(hipError_t e, const char* what) {
    return sspp::set_error(SSPP_E_NOMEM, std::string(what) + ": " + hipGetErrorString(e));
}

// device buffers, pinned buffers and events alive in this process
enum { kLiveDev = 0, kLivePinned = 1, kLiveEvents = 2 };
inline std::atomic<long long> g_live[3];
inline void live_add(int which, long long d) { g_live[which].fetch_add(d, std::memory_order_relaxed); }

template <class T>
struct Dev {
    T* p = nullptr;
    size_t n = 0;  // elements
    Dev() = default;
    Dev(Dev&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    Dev& operator=(Dev&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p; n = o.n;
            o.p = nullptr; o.n = 0;
        }
        return *this;
    }
    ~Dev() { reset(); }
    void reset() {
        if (p) { (void)hipFree(p); live_add(kLiveDev, -1); }
        p = nullptr; n = 0;
    }
    // the pointer, no longer owned
    T* release() {
        T* q = p;
        if (p) live_add(kLiveDev, -1);
        p = nullptr; n = 0;
        return q;
    }
    // room for count elements: grow only, contents not kept, no synchronisation (a caller whose
    // earlier launches may still read the buffer synchronises first)
    int reserve(size_t count) {
        if (count <= n) return SSPP_OK;
        reset();
        hipError_t e = hipMalloc((void**)&p, sizeof(T) * count);
        if (e != hipSuccess) { p = nullptr; return nomem(e, "hipMalloc"); }
        live_add(kLiveDev, 1);
        n = count;
        return SSPP_OK;
    }
    // count elements from the host, synchronously (count 0: nothing, an empty buffer stays null)
    int upload(const T* src, size_t count) {
        if (count == 0) return SSPP_OK;
        if (int rc = reserve(count)) return rc;
        return hip_fail(hipMemcpy(p, src, sizeof(T) * count, hipMemcpyHostToDevice), "hipMemcpy (upload)");
    }
    int zero() { return n ? hip_fail(hipMemset(p, 0, sizeof(T) * n), "hipMemset") : (int)SSPP_OK; }
};

template <class T>
struct Pinned {
    T* p = nullptr;
    T* d = nullptr;  // its device address (mapped memory), looked up once per allocation
    size_t n = 0;
    unsigned flags = hipHostMallocDefault;  // hipHostMalloc's, chosen by the owner
    explicit Pinned(unsigned f = hipHostMallocDefault) : flags(f) {}
    Pinned(Pinned&& o) noexcept : p(o.p), d(o.d), n(o.n), flags(o.flags) { o.p = o.d = nullptr; o.n = 0; }
    Pinned& operator=(Pinned&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p; d = o.d; n = o.n; flags = o.flags;
            o.p = o.d = nullptr; o.n = 0;
        }
        return *this;
    }
    ~Pinned() { reset(); }
    void reset() {
        if (p) { (void)hipHostFree(p); live_add(kLivePinned, -1); }
        p = d = nullptr; n = 0;
    }
    int reserve(size_t count) {
        if (count <= n) return SSPP_OK;
        reset();
        hipError_t e = hipHostMalloc((void**)&p, sizeof(T) * count, flags);
        if (e != hipSuccess) { p = nullptr; return nomem(e, "hipHostMalloc"); }
        live_add(kLivePinned, 1);
        n = count;
        return SSPP_OK;
    }
    T* dev() {
        if (!d && p) {
            void* q = nullptr;
            if (hipHostGetDevicePointer(&q, p, 0) == hipSuccess) d = (T*)q;
        }
        return d;
    }
};

// an event without timing, created at its first record
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) { reset(); ev = o.ev; o.ev = nullptr; }
        return *this;
    }
    ~Event() { reset(); }
    void reset() {
        if (ev) { (void)hipEventDestroy(ev); live_add(kLiveEvents, -1); }
        ev = nullptr;
    }
    // created, if not yet: called before asynchronous work is queued, so that none is in flight without an event
    int ensure() {
        if (ev) return SSPP_OK;
        HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        live_add(kLiveEvents, 1);
        return SSPP_OK;
    }
    int record(hipStream_t st) { int rc = ensure(); return rc ? rc : hip_fail(hipEventRecord(ev, st), "hipEventRecord"); }
    // until the last record has completed (nothing before the first)
    int wait() { return ev ? hip_fail(hipEventSynchronize(ev), "hipEventSynchronize") : (int)SSPP_OK; }
};

// Pinned bytes that asynchronous copies read, and the event recorded behind them: the owner waits
// before it rewrites the bytes, and the memory is not freed under a copy in flight.
struct Staging {
    Pinned<unsigned char> buf;
    Event ev;
    bool pending = false;
    ~Staging() { (void)ev.wait(); }
    // room for `bytes` and the event: both exist before the owner queues a copy
    int reserve(size_t bytes) { int rc = buf.reserve(bytes); return rc ? rc : ev.ensure(); }
    int wait() {
        if (!pending) return SSPP_OK;
        if (int rc = ev.wait()) return rc;
        pending = false;
        return SSPP_OK;
    }
    int record(hipStream_t st) {
        if (int rc = ev.record(st)) return rc;
        pending = true;
        return SSPP_OK;
    }
};

// device buffers of any element type, kept until the list dies
struct Retired {
    std::vector<Dev<unsigned char>> bufs;
    template <class T>
    void take(Dev<T>&& b) {
        if (!b.p) return;
        Dev<unsigned char> r;
        r.p = (unsigned char*)b.p; r.n = sizeof(T) * b.n;  // (ownership moves: the live count stays)
        b.p = nullptr; b.n = 0;
        bufs.push_back(std::move(r));
    }
};

}  // namespace sspo
