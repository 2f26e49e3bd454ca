// Host-only check of the owning types (sspp_own.h; tests/test_own_host.py builds this with g++ under
// ASan / UBSan, without the HIP runtime).  The HIP entry points the header uses are defined here on
// top of malloc: they count what is alive, log every call, can fail the k-th creating call
// (hipMalloc, hipHostMalloc, hipEventCreateWithFlags, counted together) and abort on a free or a
// destroy of something they did not hand out.  Each case prints "<name> ok"; a failed expectation
// prints its line and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "sspp_own.h"

using namespace sspo;

namespace {
std::map<void*, char> g_mem;  // 'd' device, 'h' pinned, 'e' event
std::vector<std::string> g_log;
int g_creates = 0, g_fail_at = 0;  // creating calls so far; the one to fail (0: none)
int g_mallocs = 0, g_frees = 0;    // successful hipMalloc / hipFree calls

int live(char kind) {
    int c = 0;
    for (auto& kv : g_mem) c += kv.second == kind;
    return c;
}
hipError_t create(void** out, size_t bytes, char kind, const char* name) {
    g_log.push_back(name);
    if (++g_creates == g_fail_at) { *out = nullptr; return kind == 'e' ? hipErrorInvalidValue : hipErrorOutOfMemory; }
    *out = std::malloc(bytes ? bytes : 1);
    g_mem[*out] = kind;
    return hipSuccess;
}
hipError_t destroy(void* p, char kind, const char* name) {
    g_log.push_back(name);
    auto it = g_mem.find(p);
    if (it == g_mem.end() || it->second != kind) {
        std::fprintf(stderr, "%s of a pointer that is not alive\n", name);
        std::abort();
    }
    g_mem.erase(it);
    std::free(p);
    return hipSuccess;
}
void fresh(int fail_at = 0) { g_log.clear(); g_creates = 0; g_fail_at = fail_at; g_mallocs = g_frees = 0; }
int count(const char* name) {
    int c = 0;
    for (auto& s : g_log) c += s == name;
    return c;
}
int index_of(const char* name) {
    for (size_t i = 0; i < g_log.size(); ++i) if (g_log[i] == name) return (int)i;
    return -1;
}
std::string g_err;
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    hipError_t e = create(p, n, 'd', "hipMalloc");
    g_mallocs += e == hipSuccess;
    return e;
}
hipError_t hipFree(void* p) { ++g_frees; return destroy(p, 'd', "hipFree"); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return create(p, n, 'h', "hipHostMalloc"); }
hipError_t hipHostFree(void* p) { return destroy(p, 'h', "hipHostFree"); }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { g_log.push_back("hipHostGetDevicePointer"); *d = h; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return create((void**)e, 1, 'e', "hipEventCreateWithFlags"); }
hipError_t hipEventDestroy(hipEvent_t e) { return destroy((void*)e, 'e', "hipEventDestroy"); }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { g_log.push_back("hipEventRecord"); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { g_log.push_back("hipEventSynchronize"); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { g_log.push_back("hipMemcpy"); std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemset(void* d, int v, size_t n) { g_log.push_back("hipMemset"); std::memset(d, v, n); return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

int sspp::set_error(int code, const std::string& msg) { g_err = msg; return code; }
void sspp::clear_error() { g_err.clear(); }

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

template <class B>
static bool whole_or_empty(const B& b, size_t count) {
    return (b.p == nullptr && b.n == 0) || (b.p != nullptr && b.n == count);
}
static long long lv(int which) { return g_live[which].load(); }

// the shape of sspp_job_set_queries: two device buffers, the pinned staging, its event
struct Queries {
    Dev<unsigned long long> tab;
    Dev<int> pairs;
    Staging st;
};
static int set_queries(Queries& q) {
    int rc;
    if ((rc = q.st.wait()) || (rc = q.tab.reserve(64)) || (rc = q.pairs.reserve(8)) || (rc = q.st.reserve(100)))
        return rc;
    CHECK(q.st.ev.ev != nullptr);  // the event exists before a copy would be queued
    std::memset(q.st.buf.p, 7, 100);
    return q.st.record(nullptr);
}
// the shape of run_tsp's k_tsp_pp2 records: three device buffers behind a guard on the last, zeroed
struct Records {
    Dev<unsigned> nd;
    Dev<double> term;
    Dev<unsigned> arrive;
};
static int records(Records& r) {
    if (r.arrive.p) return SSPP_OK;
    int rc;
    if ((rc = r.nd.reserve(40)) || (rc = r.term.reserve(40)) || (rc = r.arrive.reserve(10))) return rc;
    if ((rc = r.arrive.zero())) { r.arrive.reset(); return rc; }
    return SSPP_OK;
}

int main() {
    // reserve grows only: 4, 2, 8 elements are two allocations and one free
    fresh();
    {
        Dev<double> d;
        CHECK(d.reserve(4) == SSPP_OK && d.n == 4);
        double* first = d.p;
        CHECK(d.reserve(2) == SSPP_OK && d.p == first && d.n == 4);
        CHECK(d.reserve(8) == SSPP_OK && d.n == 8);
        CHECK(g_mallocs == 2 && g_frees == 1 && live('d') == 1 && lv(kLiveDev) == 1);
        double src[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        CHECK(d.upload(src, 8) == SSPP_OK && d.p[7] == 8.0 && g_mallocs == 2);
        CHECK(d.zero() == SSPP_OK && d.p[7] == 0.0);
        Dev<double> none;
        CHECK(none.upload(src, 0) == SSPP_OK && none.p == nullptr && none.zero() == SSPP_OK && g_mallocs == 2);
    }
    CHECK(live('d') == 0 && lv(kLiveDev) == 0 && g_frees == 2);
    std::printf("reserve ok\n");

    // a creation that fails at its k-th creating call, then succeeds at the second attempt
    for (int k = 1; k <= 4; ++k) {
        fresh(k);
        {
            Queries q;
            const int rc = set_queries(q);
            CHECK(rc == (k == 4 ? SSPP_E_HIP : SSPP_E_NOMEM));
            CHECK(g_creates == k);  // nothing is tried past the failure
            CHECK(whole_or_empty(q.tab, 64) && whole_or_empty(q.pairs, 8) && whole_or_empty(q.st.buf, 100));
            CHECK((q.tab.p != nullptr) == (k > 1) && (q.pairs.p != nullptr) == (k > 2) && (q.st.buf.p != nullptr) == (k > 3));
            CHECK(q.st.ev.ev == nullptr && !q.st.pending);
            CHECK(lv(kLiveDev) == live('d') && lv(kLivePinned) == live('h') && lv(kLiveEvents) == live('e'));
            g_fail_at = 0;
            CHECK(set_queries(q) == SSPP_OK);
            CHECK(q.tab.n == 64 && q.pairs.n == 8 && q.st.buf.n == 100 && q.st.ev.ev && q.st.pending);
            CHECK(live('d') == 2 && live('h') == 1 && live('e') == 1);
            CHECK(lv(kLiveDev) == 2 && lv(kLivePinned) == 1 && lv(kLiveEvents) == 1);
            CHECK(set_queries(q) == SSPP_OK && live('d') == 2 && live('h') == 1 && live('e') == 1);  // a third: waits, allocates nothing
        }
        CHECK(g_mem.empty() && lv(kLiveDev) == 0 && lv(kLivePinned) == 0 && lv(kLiveEvents) == 0);
    }
    {  // (the sweep covered every creating call of the sequence)
        fresh();
        Queries q;
        CHECK(set_queries(q) == SSPP_OK && g_creates == 4);
    }
    std::printf("set_queries sweep ok\n");

    for (int k = 1; k <= 3; ++k) {
        fresh(k);
        {
            Records r;
            CHECK(records(r) == SSPP_E_NOMEM && g_creates == k);
            CHECK(whole_or_empty(r.nd, 40) && whole_or_empty(r.term, 40) && r.arrive.p == nullptr && r.arrive.n == 0);
            g_fail_at = 0;
            CHECK(records(r) == SSPP_OK);
            CHECK(r.nd.n == 40 && r.term.n == 40 && r.arrive.n == 10 && r.arrive.p[9] == 0u);
            CHECK(g_mallocs == 3 && g_frees == 0 && live('d') == 3);  // the buffers of the first attempt are kept, none twice
            CHECK(records(r) == SSPP_OK && g_mallocs == 3 && count("hipMemset") == 1);
        }
        CHECK(g_mem.empty() && lv(kLiveDev) == 0);
    }
    {
        fresh();
        Records r;
        CHECK(records(r) == SSPP_OK && g_creates == 3);
    }
    std::printf("records sweep ok\n");

    // moves
    fresh();
    {
        Dev<int> a, b;
        CHECK(a.reserve(3) == SSPP_OK && b.reserve(5) == SSPP_OK);
        int* pa = a.p;
        Dev<int> c(std::move(a));
        CHECK(a.p == nullptr && a.n == 0 && c.p == pa && c.n == 3 && g_frees == 0);
        b = std::move(c);  // frees b's five
        CHECK(c.p == nullptr && c.n == 0 && b.p == pa && b.n == 3 && g_frees == 1 && live('d') == 1);
        Dev<int>& same = b;
        b = std::move(same);
        CHECK(b.p == pa && b.n == 3 && g_frees == 1 && live('d') == 1);
        Pinned<int> h(hipHostMallocMapped), g;
        CHECK(h.reserve(2) == SSPP_OK && h.dev() == h.p);
        g = std::move(h);
        CHECK(h.p == nullptr && h.n == 0 && g.n == 2 && g.flags == hipHostMallocMapped && live('h') == 1);
        Event e, f;
        CHECK(e.record(nullptr) == SSPP_OK);
        hipEvent_t ev = e.ev;
        f = std::move(e);
        CHECK(e.ev == nullptr && f.ev == ev && live('e') == 1);
        CHECK(lv(kLiveDev) == 1 && lv(kLivePinned) == 1 && lv(kLiveEvents) == 1);
    }
    CHECK(g_mem.empty() && lv(kLiveDev) == 0 && lv(kLivePinned) == 0 && lv(kLiveEvents) == 0);
    std::printf("moves ok\n");

    // release() leaves nothing to free; a retired buffer is freed once, when the list dies
    fresh();
    {
        int* raw = nullptr;
        {
            Dev<int> a;
            CHECK(a.reserve(3) == SSPP_OK);
            raw = a.release();
            CHECK(raw && a.p == nullptr && a.n == 0 && lv(kLiveDev) == 0);
        }
        CHECK(g_frees == 0 && live('d') == 1);
        CHECK(hipFree(raw) == hipSuccess);
        fresh();
        {
            Retired list;
            {
                Dev<double> t;
                Dev<float> empty;
                CHECK(t.reserve(6) == SSPP_OK);
                double* pt = t.p;
                list.take(std::move(t));
                list.take(std::move(empty));
                CHECK(t.p == nullptr && t.n == 0 && list.bufs.size() == 1 && (void*)list.bufs[0].p == (void*)pt);
                CHECK(list.bufs[0].n == 6 * sizeof(double));
            }
            CHECK(g_frees == 0 && live('d') == 1 && lv(kLiveDev) == 1);
        }
        CHECK(g_frees == 1 && g_mem.empty() && lv(kLiveDev) == 0);
    }
    std::printf("release and retired ok\n");

    // Staging: wait() is free without a pending copy, one synchronisation with one, and the
    // destructor synchronises the event before the pinned memory goes
    fresh();
    {
        Staging s;
        CHECK(s.wait() == SSPP_OK && g_log.empty());
        CHECK(s.reserve(16) == SSPP_OK && s.buf.n == 16 && s.ev.ev && !s.pending && count("hipEventRecord") == 0);
        CHECK(s.record(nullptr) == SSPP_OK && s.pending && count("hipEventCreateWithFlags") == 1);
        fresh();
        CHECK(s.wait() == SSPP_OK && !s.pending && g_log == std::vector<std::string>{"hipEventSynchronize"});
        CHECK(s.wait() == SSPP_OK && g_log.size() == 1);
        CHECK(s.record(nullptr) == SSPP_OK);
        fresh();
    }
    CHECK(index_of("hipEventSynchronize") >= 0 && index_of("hipEventSynchronize") < index_of("hipHostFree"));
    CHECK(index_of("hipEventDestroy") >= 0 && count("hipHostFree") == 1 && g_mem.empty());
    std::printf("staging ok\n");
    return 0;
}
