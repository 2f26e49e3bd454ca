// sspp_report.hip — the contact report: its kernels, launches and C ABI (DESIGN.md §5 "Contact report").
//
// A translation unit of its own: no scoring kernel is instantiated here, so none is rebuilt.
// The kernels are thin loops around sspr::pose_report (sspp_report.h): one lane per pose, or per
// (path, waypoint); the scene's pairs in a wave-uniform loop (the pair record is a scalar load and
// the pair-type branch is uniform, as in point_collide); each count stored when found, as a plain
// byte store into the dense [pose][pair] outputs.  No atomics, no LDS hand-shake, no early exit.
#include "sspp_report.h"

using namespace sspk;
using namespace sspr;

namespace sspr {

constexpr int kReportBlock = 256;  // 4 waves; the FP64 colliders bound the occupancy, not the block

// pose form: lane = pose
template <int NM, int MODE, int FORM>
__global__ __launch_bounds__(kReportBlock) void k_report_pose(const SceneT T, const int np, const int D,
                                                               const double* __restrict__ d_q, const long long N,
                                                               uint8_t* __restrict__ contact,
                                                               uint8_t* __restrict__ deep) {
    const long long i = (long long)blockIdx.x * kReportBlock + threadIdx.x;
    if (i >= N) return;  // (a partial last wave: nothing below votes or synchronises)
    double q[kPoseVals<NM, MODE>];
    gather_pose<NM, MODE>(d_q + i * D, D, q);
    pose_report<NM, MODE, FORM>(q, D, (cgeom_t)T.geoms, (cpair_t)T.pairs, (cmover_t)T.movers, np, contact + i * np,
                                deep ? deep + i * np : nullptr);
}

// SamplingPathPlanner path form: lane = (path b, waypoint i), u = i / W from the job's basis rows.
// eval_pt's products and fma order with the dof and degree as run-time values (every index a
// compile-time constant: the guards are wave-uniform), so the waypoints are k_sspp_c2f's bit for bit.
template <int NM>
__global__ __launch_bounds__(kReportBlock) void k_report_sspp(const SceneT T, const int np, const int D, const int P,
                                                               const int n, const int Wn,
                                                               const double* __restrict__ tab,
                                                               const int* __restrict__ span,
                                                               const double* __restrict__ ctrl, const long long total,
                                                               uint8_t* __restrict__ contact,
                                                               uint8_t* __restrict__ deep) {
    const long long idx = (long long)blockIdx.x * kReportBlock + threadIdx.x;
    if (idx >= total) return;
    const long long b = idx / Wn;
    const int i = (int)(idx - b * Wn);
    const double* N = tab + (size_t)i * (P + 1);
    const double* c0 = ctrl + (size_t)b * n * D + (size_t)(span[i] - P) * D;
    double q[kPoseVals<NM, 0>];
#pragma unroll
    for (int d = 0; d < kPoseVals<NM, 0>; ++d) {
        double acc = 0.0;
        if (d < D) {
            acc = N[0] * c0[d];
#pragma unroll
            for (int r = 1; r <= 3; ++r)
                if (r <= P) acc = fma(N[r], c0[r * D + d], acc);
        }
        q[d] = acc;
    }
    pose_report<NM, 0, kGeneric>(q, D, (cgeom_t)T.geoms, (cpair_t)T.pairs, (cmover_t)T.movers, np, contact + idx * np,
                                 deep ? deep + idx * np : nullptr);
}

// TaskSpacePlanner path form: one workgroup per via set.  tsp_prologue replays PathModel::fromVias
// (the scoring kernels' own prologue: control points bit-identical), then lane = waypoint i = 1..cp.
constexpr int kTspReportBlock = 64;
constexpr int kTspMaxN = 62;  // sspp_job_create_tsp: n_vias <= 60 (checked again at the launch)
template <int FORM>
__global__ __launch_bounds__(kTspReportBlock) void k_report_tsp(const TspK a, const SceneT T,
                                                                 const double* __restrict__ tab,
                                                                 const int* __restrict__ span,
                                                                 const double* __restrict__ Minv,
                                                                 const double* __restrict__ vias,
                                                                 uint8_t* __restrict__ contact,
                                                                 uint8_t* __restrict__ deep) {
    __shared__ double s_V[kTspMaxN * 4], s_ctrl[kTspMaxN * 4];
    const int tid = threadIdx.x, np = a.sc.npairs, cp = a.cp;
    const long long b = blockIdx.x;
    tsp_prologue(a, tsp_var(a), Minv, nullptr, nullptr, vias, nullptr, tid, kTspReportBlock, 1, b, 1, 0, s_V, s_ctrl);
    for (int i = 1 + tid; i <= cp; i += kTspReportBlock) {
        double pc[4];
        eval_pt<4, 2>(s_ctrl, tab + i * 3, span[i], pc);
        const size_t row = ((size_t)b * cp + (i - 1)) * np;
        pose_report<1, 1, FORM>(pc, 4, (cgeom_t)T.geoms, (cpair_t)T.pairs, (cmover_t)T.movers, np, contact + row,
                                deep ? deep + row : nullptr);
    }
}

static int blocks_for(long long items, int block, int* out) {
    const long long nblk = (items + block - 1) / block;
    if (nblk > 0x7fffffffll) return sspp::set_error(SSPP_E_INVAL, "contact report: too many poses for one launch");
    *out = (int)nblk;
    return SSPP_OK;
}

}  // namespace sspr

static void pair_info(const sspp_scene* s, const DPair& pr, sspp_pair_info* o) {
    const DGeom& G = s->geoms[pr.gm];
    const bool gfirst = G.orig < pr.oorig;
    o->geom1 = gfirst ? G.orig : pr.oorig;
    o->geom2 = gfirst ? pr.oorig : G.orig;
    o->moving1 = gfirst ? 1 : (pr.omover >= 0);
    o->moving2 = gfirst ? (pr.omover >= 0) : 1;
    o->margin = pr.margin;
}

extern "C" int sspp_scene_pairs(const sspp_scene* s, sspp_pair_info* out, int cap, int* n) {
    sspp::clear_error();
    if (!s || !n) return sspp::set_error(SSPP_E_INVAL, "sspp_scene_pairs: null argument");
    *n = (int)s->pairs.size();
    if (!out) return SSPP_OK;
    if (cap < *n)
        return sspp::set_error(SSPP_E_INVAL, "sspp_scene_pairs: cap = " + std::to_string(cap) + " < " +
                                                 std::to_string(*n) + " pairs");
    for (int k = 0; k < *n; ++k) pair_info(s, s->pairs[k], out + k);
    return SSPP_OK;
}

extern "C" int sspp_scene_static_pairs(const sspp_scene* s, sspp_pair_info* out, uint8_t* contact, uint8_t* deep,
                                       int cap, int* n) {
    sspp::clear_error();
    if (!s || !n) return sspp::set_error(SSPP_E_INVAL, "sspp_scene_static_pairs: null argument");
    *n = (int)s->statics.size();
    if (!out && !contact && !deep) return SSPP_OK;
    if (cap < *n)
        return sspp::set_error(SSPP_E_INVAL, "sspp_scene_static_pairs: cap = " + std::to_string(cap) + " < " +
                                                 std::to_string(*n) + " pairs");
    for (int k = 0; k < *n; ++k) {
        const sspb::StaticPair& p = s->statics[k];
        if (out) out[k] = sspp_pair_info{p.g1, p.g2, 0, 0, p.margin};
        if (contact) contact[k] = p.contact;
        if (deep) deep[k] = p.deep;
    }
    return SSPP_OK;
}

extern "C" int sspp_scene_contacts(const sspp_scene* s, const double* d_q, int64_t N, uint8_t* d_contact,
                                   uint8_t* d_deep, void* stream) {
    sspp::clear_error();
    if (!s) return sspp::set_error(SSPP_E_INVAL, "sspp_scene_contacts: null scene");
    if (N < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_scene_contacts: negative pose count");
    const int np = (int)s->pairs.size();
    if (N == 0 || np == 0) return SSPP_OK;
    if (!d_q || !d_contact) return sspp::set_error(SSPP_E_INVAL, "sspp_scene_contacts: null poses / contact output");
    int nblk = 0;
    if (int rc = blocks_for(N, kReportBlock, &nblk)) return rc;
    const KScene sc = kscene(s, s->mode == SSPP_MODE_BODY);
    const SceneT T = scene_t(s);
    dispatch_form(s->mode, (int)s->movers.size(), form_of(sc), [&](auto nm, auto mode, auto form) {
        hipLaunchKernelGGL((k_report_pose<decltype(nm)::value, decltype(mode)::value, decltype(form)::value>), dim3(nblk),
                           dim3(kReportBlock), 0, (hipStream_t)stream, T, np, s->dof, d_q, (long long)N, d_contact,
                           d_deep);
    });
    return sspo::hip_fail(hipGetLastError(), "sspp_scene_contacts launch");
}

extern "C" int sspp_job_path_contacts(sspp_job* j, const double* d_paths, int64_t B, uint8_t* d_contact,
                                      uint8_t* d_deep, void* stream) {
    sspp::clear_error();
    if (!j) return sspp::set_error(SSPP_E_INVAL, "sspp_job_path_contacts: null job");
    if (!j->bound || !j->scene)
        return sspp::set_error(SSPP_E_SCENE, "sspp_job_path_contacts: the job has no scene (none given, or freed)");
    if (B < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_job_path_contacts: negative path count");
    const sspp_scene* s = j->scene;
    const int np = (int)s->pairs.size();
    if (B == 0 || np == 0) return SSPP_OK;
    if (!d_paths || !d_contact) return sspp::set_error(SSPP_E_INVAL, "sspp_job_path_contacts: null paths / contact output");
    const SceneT T = scene_t(s);
    if (j->kind == 0) {
        const int Wn = j->W + 1;
        int nblk = 0;
        if (int rc = blocks_for((long long)B * Wn, kReportBlock, &nblk)) return rc;
        auto launch = [&](auto nm) {
            hipLaunchKernelGGL((k_report_sspp<decltype(nm)::value>), dim3(nblk), dim3(kReportBlock), 0,
                               (hipStream_t)stream, T, np, j->D, j->p, j->n, Wn, j->d_tab.p, j->d_span.p, d_paths,
                               (long long)B * Wn, d_contact, d_deep);
        };
        if (s->movers.size() > 1) launch(std::integral_constant<int, 2>{});
        else launch(std::integral_constant<int, 1>{});
    } else {
        if (B > 0x7fffffffll) return sspp::set_error(SSPP_E_INVAL, "contact report: too many paths for one launch");
        if (j->n > kTspMaxN)  // (k_report_tsp's LDS arrays)
            return sspp::set_error(SSPP_E_UNSUPPORTED, "sspp_job_path_contacts: more than " +
                                                           std::to_string(kTspMaxN - 2) + " via points");
        TspK k{};
        k.sc = kscene(s, true, j->tsp_generic != 0);
        k.n = j->n; k.K = j->K; k.cp = j->cp;
        for (int i = 0; i < 4; ++i) { k.start[i] = j->start[i]; k.end[i] = j->end[i]; }
        const int form = form_of(k.sc);
        auto launch = [&](auto f) {
            hipLaunchKernelGGL((k_report_tsp<decltype(f)::value>), dim3((int)B), dim3(kTspReportBlock), 0,
                               (hipStream_t)stream, k, T, j->d_tab.p, j->d_span.p, j->d_Minv.p, d_paths, d_contact,
                               d_deep);
        };
        if (form == kUpright) launch(std::integral_constant<int, kUpright>{});
        else if (form == kVertical) launch(std::integral_constant<int, kVertical>{});
        else launch(std::integral_constant<int, kGeneric>{});
    }
    return sspo::hip_fail(hipGetLastError(), "sspp_job_path_contacts launch");
}

// ---- the report on host buffers (the drop-in planners' contact_report / check_collision_point):
// staged to the device, run by the two calls above and copied back on the drop-in planners' shared
// stream (sspp::shared_stream(0)), which alone is waited for: other streams of the process go on
static int report_on_stream(hipStream_t st, int rc, const Dev<uint8_t>& d_c, const Dev<uint8_t>& d_d, size_t bytes,
                            uint8_t* contact, uint8_t* deep) {
    if (!rc && bytes) rc = hip_fail(hipMemcpyAsync(contact, d_c.p, bytes, hipMemcpyDeviceToHost, st), "copy contact");
    if (!rc && bytes && deep) rc = hip_fail(hipMemcpyAsync(deep, d_d.p, bytes, hipMemcpyDeviceToHost, st), "copy deep");
    // (also after a failure: the staged input and the outputs die with the caller's frame)
    const int rs = hip_fail(hipStreamSynchronize(st), "contact report");
    return rc ? rc : rs;
}

extern "C" int sspp_scene_contacts_host(const sspp_scene* s, const double* q, int64_t N, uint8_t* contact,
                                        uint8_t* deep) {
    sspp::clear_error();
    if (!s || !q || !contact || N < 1) return sspp::set_error(SSPP_E_INVAL, "sspp_scene_contacts_host: bad argument");
    hipStream_t st = (hipStream_t)sspp::shared_stream(0);
    const size_t bytes = (size_t)N * s->pairs.size(), nq = (size_t)N * s->dof;
    Dev<double> d_q;
    Dev<uint8_t> d_c, d_d;
    int rc;
    if ((rc = d_q.reserve(nq)) || (rc = d_c.reserve(bytes)) || (deep && (rc = d_d.reserve(bytes)))) return rc;
    rc = hip_fail(hipMemcpyAsync(d_q.p, q, sizeof(double) * nq, hipMemcpyHostToDevice, st), "copy poses");
    if (!rc) rc = sspp_scene_contacts(s, d_q.p, N, d_c.p, deep ? d_d.p : nullptr, st);
    return report_on_stream(st, rc, d_c, d_d, bytes, contact, deep);
}

// (a SamplingPathPlanner job is made and freed per call: a diagnostic, not a hot path)
extern "C" int sspp_path_contacts_host(const sspp_scene* s, const double* knots, int degree, const double* ctrl,
                                       int64_t B, int n, int W, uint8_t* contact, uint8_t* deep) {
    sspp::clear_error();
    if (!s || !knots || !ctrl || !contact || B < 1)
        return sspp::set_error(SSPP_E_INVAL, "sspp_path_contacts_host: bad argument");
    sspp_sspp_args a{};
    const std::vector<double> ones((size_t)s->dof, 1.0);
    a.knots = knots; a.degree = degree; a.init_ctrl = ctrl; a.n_ctrl = n; a.dof = s->dof;
    a.sigma = 0.0; a.limits = ones.data(); a.check_points = W;
    sspp_job* j = nullptr;
    int rc = sspp_job_create_sspp(s, &a, B, &j);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)sspp::shared_stream(0);
    const size_t bytes = (size_t)B * (W + 1) * s->pairs.size(), nc = (size_t)B * n * s->dof;
    {
        Dev<double> d_ctrl;
        Dev<uint8_t> d_c, d_d;
        if (!(rc = d_ctrl.reserve(nc)) && !(rc = d_c.reserve(bytes)) && !(deep && (rc = d_d.reserve(bytes)))) {
            rc = hip_fail(hipMemcpyAsync(d_ctrl.p, ctrl, sizeof(double) * nc, hipMemcpyHostToDevice, st), "copy splines");
            if (!rc) rc = sspp_job_path_contacts(j, d_ctrl.p, B, d_c.p, deep ? d_d.p : nullptr, st);
            rc = report_on_stream(st, rc, d_c, d_d, bytes, contact, deep);
        }
    }
    sspp_job_free(j);
    return rc;
}
