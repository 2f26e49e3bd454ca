// Host check of the dynamic LDS layouts in sspp_amd/csrc/sspp_lds.h, which give the host its launch
// sizes.  What the check covers on the device side differs per layout (see the header): k_sspp_census
// takes its pointers from CensusLds, and k_tsp_pp / k_tsp_pp2 walk TspPpLds' region lengths, so for
// them it holds for kernel and host alike.  k_sspp_c2f and its split epilogue form their pointers by
// hand; for C2fLds and C2fSplitLds this checks only that the host's restatement is consistent and
// sized as before, not that the kernel agrees with it.
// Sweeps D, n, p, W, nm and the candidates per workgroup of tests/test_gpu_parity.py::SHAPES, for
// sampled candidates (own rows [p, n-p)) and caller splines (own rows [0, n)): regions disjoint and
// inside `bytes`, 64-bit regions 8-byte aligned, the FP32 copies at the doubles' offsets, phase 3's
// reuse of the hull-box region inside it.  Six shapes are pinned to the byte counts of the formula
// the layouts replaced, as are the census and the two k_tsp_pp* layouts.
// Built and run by tests/test_lds_layout.py.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "sspp_lds.h"

using namespace sspk;

static int g_bad = 0;
#define CHECK(c, ...)                                      \
    do {                                                   \
        if (!(c)) {                                        \
            if (g_bad++ < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                  \
    } while (0)

struct Region { const char* name; long long at, size; };

static void disjoint_inside(std::vector<Region> r, long long bytes, const char* what) {
    std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.at < b.at; });
    long long end = 0;
    for (const Region& x : r) {
        CHECK(x.at >= end, "%s: %s at %lld overlaps the region before it (ends %lld)", what, x.name, x.at, end);
        end = x.at + x.size;
    }
    CHECK(end <= bytes, "%s: regions end at %lld past bytes %lld", what, end, bytes);
}

static long long check_c2f(int n, int D, int cpb, int nrd, int nm, int lpc) {
    const C2fLds l = c2f_layout(n, D, cpb, nrd, nm, lpc);
    const int ndof = n * D, nvw3 = lpc / 64, nf = ndof + cpb * nrd;
    char what[96];
    std::snprintf(what, sizeof what, "c2f n %d D %d cpb %d nrd %d nm %d lpc %d", n, D, cpb, nrd, nm, lpc);
    disjoint_inside({{"fix", 8LL * l.fix, 8LL * ndof},
                     {"own", 8LL * l.own, 8LL * cpb * nrd},
                     {"lim", 8LL * l.lim, 8LL * D},
                     {"box", 8LL * l.box, 8LL * cpb * l.rbox},
                     {"mask", l.mask, 8LL * cpb},
                     {"feas", l.feas, 4LL * cpb},
                     {"surv", l.surv, 4LL * (cpb + 1)},
                     {"defer", l.defer, 4LL * cpb},
                     {"f32", l.f32, 4LL * nf}},
                    l.bytes, what);
    CHECK(l.mask % 8 == 0, "%s: mask at %d", what, l.mask);  // (the double regions are 8 x an index)
    CHECK(l.feas % 4 == 0 && l.surv % 4 == 0 && l.defer % 4 == 0 && l.f32 % 4 == 0, "%s: 32-bit regions", what);
    // the FP32 copies mirror the doubles: the kernel indexes them with fix and own
    CHECK(l.fix == 0 && l.own == ndof && l.own + cpb * nrd == nf, "%s: FP32 mirror", what);
    CHECK(l.f32 + 4LL * nf == l.bytes, "%s: FP32 copies end at bytes", what);
    // phase 2's hull boxes [cpb][2][3 nm]; phase 3's group sums [cpb][lpc / 64] then arcs [cpb]
    CHECK(2 * 3 * nm <= l.rbox, "%s: hull boxes need %d of rbox %d", what, 6 * nm, l.rbox);
    CHECK(l.arc == l.box + cpb * nvw3, "%s: arcs follow the group sums", what);
    CHECK(l.arc + cpb <= l.box + cpb * l.rbox, "%s: phase 3 needs %d doubles of %d", what, cpb * (nvw3 + 1), cpb * l.rbox);
    return l.bytes;
}

int main() {
    const int Ds[] = {1, 2, 3, 4, 6, 7, 9}, Ws[] = {2, 50, 128, 256};
    const int cpbs[] = {32, 16, 21, 8, 4, 1};  // (nt / 64) * (64 / g1) of test_gpu_parity.py::SHAPES
    long long cases = 0;
    for (int D : Ds)
        for (int n = 4; n <= 16; ++n)
            for (int p = 2; p <= 3; ++p)
                for (int W : Ws)
                    for (int nm = 1; nm <= 2; ++nm)
                        for (int cpb : cpbs) {
                            const int r0 = std::min(p, n), r1 = std::max(r0, n - p);
                            check_c2f(n, D, cpb, (r1 - r0) * D, nm, lanes_for(W - 1));  // sampled
                            check_c2f(n, D, cpb, n * D, nm, lanes_for(W - 1));          // caller splines
                            const CensusLds c = census_layout(n, D, (r1 - r0) * D);
                            disjoint_inside({{"fix", 8LL * c.fix, 8LL * n * D},
                                             {"own", 8LL * c.own, 8LL * (r1 - r0) * D},
                                             {"lim", 8LL * c.lim, 8LL * D}},
                                            c.bytes, "census");
                            cases += 2;
                        }
    // the byte counts of the formulas the layouts replaced (c2f_lds, launch_census, entry_tsp)
    CHECK(check_c2f(10, 7, 32, 28, 1, lanes_for(127)) == 13828, "pinned c2f 1");
    CHECK(check_c2f(10, 7, 4, 70, 1, lanes_for(127)) == 4532, "pinned c2f 2");
    CHECK(check_c2f(4, 1, 1, 0, 1, lanes_for(1)) == 128, "pinned c2f 3");
    CHECK(check_c2f(16, 9, 16, 90, 2, lanes_for(255)) == 20940, "pinned c2f 4");
    CHECK(check_c2f(8, 4, 21, 16, 1, lanes_for(49)) == 5880, "pinned c2f 5");
    CHECK(check_c2f(12, 6, 8, 72, 1, lanes_for(255)) == 8372, "pinned c2f 6");
    CHECK(census_layout(10, 7, 28).bytes == 840, "pinned census 1");
    CHECK(census_layout(4, 1, 0).bytes == 40, "pinned census 2");
    CHECK(census_layout(16, 9, 90).bytes == 1944, "pinned census 3");
    const int ns[] = {4, 7, 16}, pp[] = {37120, 37312, 37888}, pp2[] = {256, 448, 1024};
    for (int i = 0; i < 3; ++i) {
        const TspPpLds a = tsp_pp_layout(ns[i], true), b = tsp_pp_layout(ns[i], false);
        CHECK(a.bytes == pp[i] && b.bytes == pp2[i], "pinned k_tsp_pp* n %d: %d %d", ns[i], a.bytes, b.bytes);
        // the kernels walk the lengths: vias, control points and terms are doubles (so the counts
        // start 8-byte aligned: they are cleared as 32-bit words), the counts bytes
        CHECK(a.n_V == 4 * ns[i] && a.n_ctrl == 4 * ns[i] && a.n_term == 64 * 64 && a.n_nd == 64 * 64, "k_tsp_pp lengths");
        CHECK(b.n_V == 4 * ns[i] && b.n_ctrl == 4 * ns[i] && b.n_term == 0 && b.n_nd == 0, "k_tsp_pp2 lengths");
        CHECK(a.bytes == 8 * (a.n_V + a.n_ctrl + a.n_term) + a.n_nd, "k_tsp_pp: bytes is the walk's end");
    }
    // the split epilogue: 64-bit regions aligned, everything inside the 20 * kMaxSteps + 16 bytes
    const C2fSplitLds s = c2f_split_layout();
    disjoint_inside({{"bits", s.bits, 8LL * kMaxSteps}, {"id", s.id, 8LL * kMaxSteps}, {"cnt", s.cnt, 4LL * kMaxSteps},
                     {"lost", s.lost, 4}}, s.bytes, "split epilogue");
    CHECK(s.bits % 8 == 0 && s.id % 8 == 0 && s.cnt % 4 == 0 && s.lost % 4 == 0, "split epilogue alignment");
    CHECK(s.bytes == 20 * kMaxSteps + 16 && s.bytes == 1296, "pinned split epilogue: %d", s.bytes);
    std::printf("layouts checked %lld failures %d\n", cases, g_bad);
    return g_bad ? 1 : 0;
}
