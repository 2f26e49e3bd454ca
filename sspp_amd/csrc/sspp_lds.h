// sspp_lds.h — the dynamic LDS layouts of the kernels (sspp_kern.h) and the host's byte counts for
// their launches.  Plain C++ (tests/lds_layout/check_layout.cpp compiles it on the host).
// Who reads what:
//   * CensusLds: k_sspp_census takes its pointers from the offsets; launch_census the bytes.
//   * TspPpLds: k_tsp_pp and k_tsp_pp2 form their pointers by walking the region lengths in order;
//     entry_tsp takes the bytes.
//   * C2fLds, C2fSplitLds: the host only (c2f_lds, run_sspp's split launch).  k_sspp_c2f and its split
//     epilogue form their pointers by hand in the same order — taking them from these structs moved
//     the kernel's register allocation — so these two restate the kernel's chain and nothing checks
//     them against it: an edit to one is an edit to the other.
// tsp_body's DEF layouts (tsp_base_lds, tsp_def_lds, tsp_def2_lds: sspp_kern.h) are not here.
#pragma once
#if defined(__HIPCC__)
#define SSPP_LDS_HD __host__ __device__
#else
#define SSPP_LDS_HD
#endif

namespace sspk {

constexpr int kBlock = 256;    // threads per workgroup (k_tsp; the argmin's default)
constexpr int kMaxSteps = 64;  // steps per launch (k_sspp_c2f)

// lanes that share a candidate's items: a multiple of 64, at least 64, at most a workgroup
inline int lanes_for(int items) {
    const int l = ((items + 63) / 64) * 64;
    return l < 64 ? 64 : (l > kBlock ? kBlock : l);
}

// k_sspp_c2f (read by the host only, see above): n control points of D doubles, cpb candidates per workgroup of nrd own doubles each,
// NM movers, lpc canonical lanes of the arc-length sum.  fix .. arc count doubles from the start of
// the dynamic LDS; fix and own also index the FP32 copies from f32 (same offsets as the doubles);
// mask .. f32 and bytes count bytes.
struct C2fLds {
    int fix;    // [n][D]          the shared initial spline
    int own;    // [cpb][nrd]      the candidates' own rows
    int lim;    // [D]             sampleWithNoise limits
    int box;    // [cpb][rbox]     hull boxes [cpb][2][3 NM] (phase 2), reused by phase 3:
    int arc;    //                 group sums [cpb][lpc / 64] at box, then arc lengths [cpb] at arc
    int rbox;   // doubles per candidate of that region: max(2 * 3 NM, lpc / 64 + 1)
    int mask;   // [cpb] 64-bit    hull masks
    int feas;   // [cpb] int       feasible flags
    int surv;   // [cpb + 1] int   survivor list (last = count)
    int defer;  // [cpb] int       undecided cylinder-box / capsule pair
    int f32;    // [n D + cpb nrd] float copies of fix and own
    int bytes;
};
SSPP_LDS_HD inline C2fLds c2f_layout(int n, int D, int cpb, int nrd, int NM, int lpc) {
    C2fLds l;
    const int ndof = n * D, nvw3 = lpc >> 6, NB = 3 * NM;
    l.fix = 0;
    l.own = ndof;
    l.lim = l.own + cpb * nrd;
    l.box = l.lim + D;
    l.arc = l.box + cpb * nvw3;
    l.rbox = 2 * NB > nvw3 + 1 ? 2 * NB : nvw3 + 1;
    l.mask = 8 * (l.box + cpb * l.rbox);
    l.feas = l.mask + 8 * cpb;
    l.surv = l.feas + 4 * cpb;
    l.defer = l.surv + 4 * (cpb + 1);
    l.f32 = l.defer + 4 * cpb;
    l.bytes = l.f32 + 4 * (ndof + cpb * nrd);
    return l;
}

// (host only, see above) the epilogue of a split k_sspp_c2f launch (its last workgroup) reuses the LDS from offset 0: per
// step the minimum arc's bits, its lowest id and the feasible count, then the lost survivors
struct C2fSplitLds {
    int bits;  // [kMaxSteps] 64-bit
    int id;    // [kMaxSteps] 64-bit
    int cnt;   // [kMaxSteps] unsigned
    int lost;  // [1] unsigned (padded to 16 bytes)
    int bytes;
};
SSPP_LDS_HD inline C2fSplitLds c2f_split_layout() {
    C2fSplitLds l;
    l.bits = 0;
    l.id = l.bits + 8 * kMaxSteps;
    l.cnt = l.id + 8 * kMaxSteps;
    l.lost = l.cnt + 4 * kMaxSteps;
    l.bytes = l.lost + 16;
    return l;
}

// k_sspp_census: the initial spline, one candidate's own rows, the limits (doubles)
struct CensusLds {
    int fix, own, lim, bytes;
};
SSPP_LDS_HD inline CensusLds census_layout(int n, int D, int nrd) {
    CensusLds l;
    l.fix = 0;
    l.own = n * D;
    l.lim = l.own + nrd;
    l.bytes = 8 * (l.lim + D);
    return l;
}

// k_tsp_pp (rec: with the per-(waypoint, pair) records in LDS) and k_tsp_pp2 (records in global
// memory): the regions' lengths in elements, in LDS order — the kernels form their pointers by
// walking them, each region starting where the one before it ends: one candidate's vias [n][4]
// and control points [n][4] (doubles), then the terms [64][64] (doubles) and the counts [64][64]
// (bytes).
struct TspPpLds {
    int n_V, n_ctrl, n_term, n_nd;
    int bytes;
};
SSPP_LDS_HD inline TspPpLds tsp_pp_layout(int n, bool rec) {
    TspPpLds l;
    l.n_V = n * 4;
    l.n_ctrl = n * 4;
    l.n_term = rec ? 64 * 64 : 0;
    l.n_nd = rec ? 64 * 64 : 0;
    l.bytes = 8 * (l.n_V + l.n_ctrl + l.n_term) + l.n_nd;
    return l;
}

}  // namespace sspk
