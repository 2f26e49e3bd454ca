// sspp_chain_report.hip — the contact report for arms: its kernels, launches and C ABI (DESIGN.md §5
// "Contact report for arms").
//
// A translation unit of its own: no existing kernel is instantiated here, so none is rebuilt.  The
// kernels are thin loops around sspc::chain_fk and sspc::chain_pair_report / chain_first_pair
// (sspp_chain_report.h).  As in sspp_chain.hip: one wave per workgroup, a lane's driven-body frames
// in dynamic LDS laid out [slot][component][lane], wave-uniform body / joint / pair loops (records
// are scalar loads), no per-lane array indexed at run time.
//   k_chain_pair_contacts  lane = pose: the report row [i][0..P)
//   k_chain_path_contacts  lane = (path, waypoint): k_chain_feas's evaluator, the row [b][i][0..P)
//   k_chain_first          one wave per path, lanes = waypoints in passes of 64; after a pass a
//                          ballot picks the lowest lane with a hit and a shuffle reads its pair; the
//                          wave stops at the first pass with a hit.  No atomics
// Stores of the two dense kernels: a lane's row is P <= 512 bytes, so plain byte stores would be
// strided by P across the lanes (64 cache lines per store instruction).  A wave's 64 rows are one
// contiguous block of the output, so the lanes write their rows into an LDS image of that block and
// the wave copies it out in 16-byte stores, lane after lane (bytes before the first and after the
// last 16-byte boundary of the block singly).  The image is shifted by the block's address modulo 16,
// so that the 16-byte reads of LDS are aligned where the stores are.
// Lanes past the end of a partial wave skip the work, not the barrier, the vote or the copy.
#include "sspp_chain_dev.h"
#include "sspp_chain_report.h"

using namespace sspk;
using namespace sspc;

namespace sspc {

// bytes of one LDS image: 64 rows of np bytes behind a shift of up to 15, a multiple of 16
__host__ __device__ inline size_t stage_bytes(int np) { return ((size_t)kChainBlock * np + 15 + 15) / 16 * 16; }
static_assert(sizeof(double) * 7 * kChainBlock * kMaxBodies + 2 * (((size_t)kChainBlock * kMaxPairs + 30) / 16 * 16) <=
                  160 * 1024, "the frames and both images of the largest chain fit a CU's LDS");
inline size_t report_lds(int nd, int np, bool deep) { return chain_lds(nd) + stage_bytes(np) * (deep ? 2 : 1); }

// the wave's block dst[0, nbytes) from its image: dst + j <-> img[pad + j], pad = dst's address mod 16
__device__ __forceinline__ void copy_out(const uint8_t* img, int pad, uint8_t* __restrict__ dst, int nbytes, int lane) {
    const int head = min(nbytes, (16 - pad) & 15);
    const int nvec = (nbytes - head) >> 4;
    const int tail0 = head + (nvec << 4);
    if (lane < head) dst[lane] = img[pad + lane];
    for (int v = lane; v < nvec; v += kChainBlock)
        *reinterpret_cast<uint4*>(dst + head + (v << 4)) = *reinterpret_cast<const uint4*>(img + pad + head + (v << 4));
    if (lane < nbytes - tail0) dst[tail0 + lane] = img[pad + tail0 + lane];
}

// the lane's report row from its frames into the wave's images, then the copy: every lane of the
// wave calls it (active: the lane has a pose); row0: the wave's first row, rows: how many it has
__device__ __forceinline__ void report_rows(const ChainT& T, const LdsFrames& fr, double* s_fr, bool active,
                                            long long row0, int rows, uint8_t* __restrict__ contact,
                                            uint8_t* __restrict__ deep) {
    const int lane = threadIdx.x, np = T.np;
    uint8_t* img_c = reinterpret_cast<uint8_t*>(s_fr + 7 * kChainBlock * max(1, T.nd));
    uint8_t* img_d = img_c + stage_bytes(np);
    uint8_t* dst_c = contact + (size_t)row0 * np;
    uint8_t* dst_d = deep ? deep + (size_t)row0 * np : nullptr;
    const int pad_c = (int)(reinterpret_cast<uintptr_t>(dst_c) & 15);
    const int pad_d = (int)(reinterpret_cast<uintptr_t>(dst_d) & 15);
    if (active)
        chain_pair_report((ccgeom_t)T.geoms, (ccpair_t)T.pairs, np, fr, img_c + pad_c + lane * np,
                          deep ? img_d + pad_d + lane * np : nullptr);
    __syncthreads();  // (one wave: the rows of the other lanes are in LDS)
    copy_out(img_c, pad_c, dst_c, rows * np, lane);
    if (deep) copy_out(img_d, pad_d, dst_d, rows * np, lane);
}

__global__ __launch_bounds__(kChainBlock) void k_chain_pair_contacts(const ChainT T, const double* __restrict__ d_q,
                                                                      const long long N,
                                                                      uint8_t* __restrict__ contact,
                                                                      uint8_t* __restrict__ deep) {
    extern __shared__ __align__(16) double s_fr[];
    const long long row0 = (long long)blockIdx.x * kChainBlock;
    const long long i = row0 + threadIdx.x;
    const LdsFrames fr{s_fr + threadIdx.x};
    const bool active = i < N;
    if (active) {
        const double* q = d_q + i * T.D;
        chain_fk((cbody_t)T.bodies, (cjoint_t)T.joints, T.nd, T.D, [q](int adr) { return q[adr]; }, fr);
    }
    report_rows(T, fr, s_fr, active, row0, (int)min((long long)kChainBlock, N - row0), contact, deep);
}

// lane = (path b, waypoint i) at u = i / W from the job's basis rows (tab: P + 1 values per
// waypoint, span: its knot span), k_chain_feas's evaluator: eval_pt's products and fma order
__global__ __launch_bounds__(kChainBlock) void k_chain_path_contacts(const ChainT T, const int P, const int n,
                                                                      const int Wn, const double* __restrict__ tab,
                                                                      const int* __restrict__ span,
                                                                      const double* __restrict__ ctrl,
                                                                      const long long total,
                                                                      uint8_t* __restrict__ contact,
                                                                      uint8_t* __restrict__ deep) {
    extern __shared__ __align__(16) double s_fr[];
    const long long row0 = (long long)blockIdx.x * kChainBlock;
    const long long idx = row0 + threadIdx.x;
    const LdsFrames fr{s_fr + threadIdx.x};
    const int D = T.D;
    const bool active = idx < total;
    if (active) {
        const long long b = idx / Wn;
        const int i = (int)(idx - b * Wn);
        const double* N = tab + (size_t)i * (P + 1);
        double Nr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) Nr[r] = r <= P ? N[r] : 0.0;
        const double* c0 = ctrl + (size_t)b * n * D + (size_t)(span[i] - P) * D;
        auto qv = [&](int adr) {
            double acc = Nr[0] * c0[adr];
#pragma unroll
            for (int r = 1; r <= 3; ++r)
                if (r <= P) acc = fma(Nr[r], c0[r * D + adr], acc);
            return acc;
        };
        chain_fk((cbody_t)T.bodies, (cjoint_t)T.joints, T.nd, D, qv, fr);
    }
    report_rows(T, fr, s_fr, active, row0, (int)min((long long)kChainBlock, total - row0), contact, deep);
}

// One wave per path b: waypoint i = pass * 64 + lane.  first[b] = {lowest waypoint in contact, its
// lowest column}, {-1, -1} for a path that touches nothing.
__global__ __launch_bounds__(kChainBlock) void k_chain_first(const ChainT T, const int P, const int n, const int W,
                                                              const double* __restrict__ tab,
                                                              const int* __restrict__ span,
                                                              const double* __restrict__ ctrl,
                                                              sspp_chain_first* __restrict__ first) {
    extern __shared__ __align__(16) double s_fr[];
    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    const LdsFrames fr{s_fr + lane};
    const int D = T.D;
    int wp = -1, col = -1;
    for (int base = 0; base <= W; base += kChainBlock) {
        const int i = base + lane;
        int pr = -1;
        if (i <= W) {
            const double* N = tab + (size_t)i * (P + 1);
            double Nr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) Nr[r] = r <= P ? N[r] : 0.0;
            const double* c0 = ctrl + (size_t)b * n * D + (size_t)(span[i] - P) * D;
            auto qv = [&](int adr) {
                double acc = Nr[0] * c0[adr];
#pragma unroll
                for (int r = 1; r <= 3; ++r)
                    if (r <= P) acc = fma(Nr[r], c0[r * D + adr], acc);
                return acc;
            };
            chain_fk((cbody_t)T.bodies, (cjoint_t)T.joints, T.nd, D, qv, fr);
            pr = chain_first_pair((ccgeom_t)T.geoms, (ccpair_t)T.pairs, T.np, fr);
        }
        const unsigned long long hits = __ballot(pr >= 0);  // wave-uniform: every lane votes
        if (hits) {
            const int src = __ffsll((long long)hits) - 1;  // the lowest lane: the lowest waypoint of the pass
            wp = base + src;
            col = __shfl(pr, src);
            break;
        }
    }
    if (lane == 0) first[b] = sspp_chain_first{wp, col};
}

// the path forms' arguments past the chain and the batch, and the scene-less job of the shape
static int path_job(sspp_chain* c, const char* who, const double* knots, int degree, int n, int W) {
    if (n < 1 || W < 1)
        return sspp::set_error(SSPP_E_INVAL, std::string(who) + ": n_ctrl and check_points must be >= 1");
    return chain_job(c, knots, degree, n, W, 1);  // (the basis rows only: any batch capacity serves)
}

}  // namespace sspc

extern "C" int sspp_chain_static_pairs(const sspp_chain* c, sspp_pair_info* out, uint8_t* contact, uint8_t* deep,
                                       int cap, int* n) {
    sspp::clear_error();
    if (!c || !n) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_static_pairs: null argument");
    *n = (int)c->t.statics.size();
    if (!out && !contact && !deep) return SSPP_OK;
    if (cap < *n)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_static_pairs: cap = " + std::to_string(cap) + " < " +
                                                 std::to_string(*n) + " pairs");
    for (int k = 0; k < *n; ++k) {
        const CStatic& p = c->t.statics[k];
        if (out) out[k] = sspp_pair_info{p.g1, p.g2, 0, 0, p.margin};
        if (contact) contact[k] = p.contact;
        if (deep) deep[k] = p.deep;
    }
    return SSPP_OK;
}

extern "C" int sspp_chain_pair_contacts(const sspp_chain* c, const double* d_q, int64_t N, uint8_t* d_contact,
                                        uint8_t* d_deep, void* stream) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_pair_contacts: null chain");
    if (N < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_pair_contacts: negative pose count");
    const ChainT T = c->view();
    if (N == 0 || T.np == 0) return SSPP_OK;
    if (!d_q || !d_contact) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_pair_contacts: null poses / contact output");
    int nblk = 0;
    if (int rc = chain_blocks(N, "sspp_chain_pair_contacts", &nblk)) return rc;
    hipLaunchKernelGGL(k_chain_pair_contacts, dim3(nblk), dim3(kChainBlock), report_lds(T.nd, T.np, d_deep != nullptr),
                       (hipStream_t)stream, T, d_q, (long long)N, d_contact, d_deep);
    return sspo::hip_fail(hipGetLastError(), "sspp_chain_pair_contacts launch");
}

extern "C" int sspp_chain_path_contacts(sspp_chain* c, const double* knots, int degree, const double* d_ctrl, int64_t B,
                                        int n, int W, uint8_t* d_contact, uint8_t* d_deep, void* stream) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_path_contacts: null chain");
    if (B < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_path_contacts: negative path count");
    const ChainT T = c->view();
    if (B == 0 || T.np == 0) return SSPP_OK;
    if (!d_ctrl || !d_contact) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_path_contacts: null paths / contact output");
    if (int rc = path_job(c, "sspp_chain_path_contacts", knots, degree, n, W)) return rc;
    const sspp_job* j = c->job;
    const int Wn = j->W + 1;
    if (B > 0x7fffffffll * kChainBlock / Wn)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_path_contacts: too many poses for one launch");
    int nblk = 0;
    if (int rc = chain_blocks(B * Wn, "sspp_chain_path_contacts", &nblk)) return rc;
    hipLaunchKernelGGL(k_chain_path_contacts, dim3(nblk), dim3(kChainBlock), report_lds(T.nd, T.np, d_deep != nullptr),
                       (hipStream_t)stream, T, j->p, j->n, Wn, j->d_tab.p, j->d_span.p, d_ctrl, (long long)B * Wn,
                       d_contact, d_deep);
    return sspo::hip_fail(hipGetLastError(), "sspp_chain_path_contacts launch");
}

extern "C" int sspp_chain_first_contacts(sspp_chain* c, const double* knots, int degree, const double* d_ctrl, int64_t B,
                                         int n, int W, sspp_chain_first* d_first, void* stream) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_first_contacts: null chain");
    if (B < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_first_contacts: negative path count");
    if (B == 0) return SSPP_OK;
    if (!d_first) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_first_contacts: null output");
    const ChainT T = c->view();
    if (T.np == 0)  // nothing can touch: every record {-1, -1}, without a launch
        return sspo::hip_fail(hipMemsetAsync(d_first, 0xff, sizeof(sspp_chain_first) * (size_t)B, (hipStream_t)stream),
                              "sspp_chain_first_contacts fill");
    if (!d_ctrl) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_first_contacts: null paths");
    if (B > 0x7fffffffll) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_first_contacts: too many paths for one launch");
    if (int rc = path_job(c, "sspp_chain_first_contacts", knots, degree, n, W)) return rc;
    const sspp_job* j = c->job;
    hipLaunchKernelGGL(k_chain_first, dim3((int)B), dim3(kChainBlock), chain_lds(T.nd), (hipStream_t)stream, T, j->p, j->n,
                       j->W, j->d_tab.p, j->d_span.p, d_ctrl, d_first);
    return sspo::hip_fail(hipGetLastError(), "sspp_chain_first_contacts launch");
}

// ---- the same on host buffers: staged to the device, run by the calls above and copied back on the
// drop-in planners' shared stream (sspp::shared_stream(0)), which alone is waited for
static int report_back(hipStream_t st, int rc, const Dev<uint8_t>& d_c, const Dev<uint8_t>& d_d, size_t bytes,
                       uint8_t* contact, uint8_t* deep) {
    if (!rc && bytes) rc = hip_fail(hipMemcpyAsync(contact, d_c.p, bytes, hipMemcpyDeviceToHost, st), "copy contact");
    if (!rc && bytes && deep) rc = hip_fail(hipMemcpyAsync(deep, d_d.p, bytes, hipMemcpyDeviceToHost, st), "copy deep");
    return chain_wait(st, rc, "chain contact report");
}

extern "C" int sspp_chain_pair_contacts_host(const sspp_chain* c, const double* q, int64_t N, uint8_t* contact,
                                             uint8_t* deep) {
    sspp::clear_error();
    if (!c || N < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_pair_contacts_host: bad argument");
    const size_t bytes = (size_t)N * c->t.pairs.size(), nq = (size_t)N * c->t.D;
    if (bytes == 0) return SSPP_OK;
    if (!q || !contact) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_pair_contacts_host: null poses / contact output");
    hipStream_t st = (hipStream_t)sspp::shared_stream(0);
    Dev<double> d_q;
    Dev<uint8_t> d_c, d_d;
    int rc;
    if ((rc = d_q.reserve(nq)) || (rc = d_c.reserve(bytes)) || (deep && (rc = d_d.reserve(bytes)))) return rc;
    rc = hip_fail(hipMemcpyAsync(d_q.p, q, sizeof(double) * nq, hipMemcpyHostToDevice, st), "copy poses");
    if (!rc) rc = sspp_chain_pair_contacts(c, d_q.p, N, d_c.p, deep ? d_d.p : nullptr, st);
    return report_back(st, rc, d_c, d_d, bytes, contact, deep);
}

extern "C" int sspp_chain_path_contacts_host(sspp_chain* c, const double* knots, int degree, const double* ctrl,
                                             int64_t B, int n, int W, uint8_t* contact, uint8_t* deep) {
    sspp::clear_error();
    if (!c || B < 0 || n < 1 || W < 1) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_path_contacts_host: bad argument");
    const size_t bytes = (size_t)B * ((size_t)W + 1) * c->t.pairs.size(), nc = (size_t)B * n * c->t.D;
    if (bytes == 0) return SSPP_OK;
    if (!knots || !ctrl || !contact)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_path_contacts_host: null knots / paths / contact output");
    hipStream_t st = (hipStream_t)sspp::shared_stream(0);
    Dev<double> d_ctrl;
    Dev<uint8_t> d_c, d_d;
    int rc;
    if ((rc = d_ctrl.reserve(nc)) || (rc = d_c.reserve(bytes)) || (deep && (rc = d_d.reserve(bytes)))) return rc;
    rc = hip_fail(hipMemcpyAsync(d_ctrl.p, ctrl, sizeof(double) * nc, hipMemcpyHostToDevice, st), "copy splines");
    if (!rc) rc = sspp_chain_path_contacts(c, knots, degree, d_ctrl.p, B, n, W, d_c.p, deep ? d_d.p : nullptr, st);
    return report_back(st, rc, d_c, d_d, bytes, contact, deep);
}

extern "C" int sspp_chain_first_contacts_host(sspp_chain* c, const double* knots, int degree, const double* ctrl,
                                              int64_t B, int n, int W, sspp_chain_first* first) {
    sspp::clear_error();
    if (!c || B < 0 || n < 1 || W < 1) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_first_contacts_host: bad argument");
    if (B == 0) return SSPP_OK;
    if (!knots || !ctrl || !first)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_first_contacts_host: null knots / paths / output");
    hipStream_t st = (hipStream_t)sspp::shared_stream(0);
    const size_t nc = (size_t)B * n * c->t.D;
    Dev<double> d_ctrl;
    Dev<sspp_chain_first> d_f;
    int rc;
    if ((rc = d_ctrl.reserve(nc)) || (rc = d_f.reserve((size_t)B))) return rc;
    rc = hip_fail(hipMemcpyAsync(d_ctrl.p, ctrl, sizeof(double) * nc, hipMemcpyHostToDevice, st), "copy splines");
    if (!rc) rc = sspp_chain_first_contacts(c, knots, degree, d_ctrl.p, B, n, W, d_f.p, st);
    if (!rc) rc = hip_fail(hipMemcpyAsync(first, d_f.p, sizeof(sspp_chain_first) * (size_t)B, hipMemcpyDeviceToHost, st), "copy first contacts");
    return chain_wait(st, rc, "sspp_chain_first_contacts_host");
}
