// sspp_chain.hip — articulated movers: the chain's kernels, launches and C ABI (DESIGN.md §5
// "Articulated movers").
//
// A translation unit of its own: no scoring kernel is instantiated here, so none is rebuilt.  The
// kernels are thin loops around sspc::chain_fk / geom_pose / chain_contact (sspp_chain.h).  A lane
// holds one pose; its driven bodies' frames live in dynamic LDS laid out [slot][component][lane]
// (consecutive lanes, consecutive 8-byte words; sized from the chain's driven-body count), so no
// per-lane array is indexed at run time.  The body, joint and pair loops are wave-uniform: records
// are scalar loads and the type branches are uniform.
//   k_chain_fk        lane = pose: every geom's world pose
//   k_chain_contacts  lane = pose: one byte
//   k_chain_feas      one wave per candidate, lanes = waypoints in passes of 64 with a wave vote
//                     after each pass: a candidate stops at its first contact (checkCollision's
//                     semantics, no atomics).  A waypoint's coordinates are evaluated when a joint
//                     asks for them, with eval_pt's products and fma order
//   k_chain_best_q    findBestPath over a batch, one workgroup: lowest arc, lowest id on ties, the
//                     feasible count; in a query launch one workgroup per query, and the winner's
//                     control points gathered into the query's row
// Arc lengths and sampled candidates come from a scene-less SamplingPathPlanner job (k_sspp_c2f,
// arc_all = 1): the existing code, bit for bit.
#include "sspp_chain_dev.h"

using namespace sspk;
using namespace sspc;

namespace sspc {

__global__ __launch_bounds__(kChainBlock) void k_chain_fk(const ChainT T, const double* __restrict__ d_q,
                                                           const long long N, double* __restrict__ gpos,
                                                           double* __restrict__ gmat) {
    extern __shared__ double s_fr[];
    const long long i = (long long)blockIdx.x * kChainBlock + threadIdx.x;
    if (i >= N) return;  // (nothing below votes or synchronises)
    const LdsFrames fr{s_fr + threadIdx.x};
    const double* q = d_q + i * T.D;
    chain_fk((cbody_t)T.bodies, (cjoint_t)T.joints, T.nd, T.D, [q](int adr) { return q[adr]; }, fr);
    for (int g = 0; g < T.ng; ++g) {
        double p[3], m[9];
        geom_pose((ccgeom_t)T.geoms + g, fr, p, m);
        double* op = gpos + ((size_t)i * T.ng + g) * 3;
        double* om = gmat + ((size_t)i * T.ng + g) * 9;
#pragma unroll
        for (int k = 0; k < 3; ++k) op[k] = p[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) om[k] = m[k];
    }
}

__global__ __launch_bounds__(kChainBlock) void k_chain_contacts(const ChainT T, const int static_block,
                                                                 const double* __restrict__ d_q, const long long N,
                                                                 uint8_t* __restrict__ hit) {
    extern __shared__ double s_fr[];
    const long long i = (long long)blockIdx.x * kChainBlock + threadIdx.x;
    if (i >= N) return;
    const LdsFrames fr{s_fr + threadIdx.x};
    const double* q = d_q + i * T.D;
    chain_fk((cbody_t)T.bodies, (cjoint_t)T.joints, T.nd, T.D, [q](int adr) { return q[adr]; }, fr);
    const int h = chain_contact((ccgeom_t)T.geoms, (ccpair_t)T.pairs, T.np, fr);
    hit[i] = (uint8_t)((h || static_block) ? 1 : 0);
}

// One wave per candidate b: waypoint i = pass * 64 + lane at u = i / W, from the job's basis rows
// (tab: P + 1 values per waypoint, span: its knot span).  Writes feasible[b], and +inf over an
// infeasible candidate's arc length.
// WORLDS (a worlds launch, DESIGN.md §5 "Worlds for arms"): candidate b belongs to query b / B, which
// is wave-uniform; T's body, joint and geom tables are [Q][nd], [Q][nj], [Q][ng] and their bases are
// offset by the query (still scalar loads from the constant address space; the pair table is
// shared), and the static block is bit b / B of static_mask.  A compile-time flag: the plain
// kernel's code is what it was.
template <bool WORLDS>
__device__ __forceinline__ void chain_feas(const ChainT& T, const unsigned long long static_mask, const int nj,
                                           const unsigned B, const int P, const int n, const int W,
                                           const double* __restrict__ tab, const int* __restrict__ span,
                                           const double* __restrict__ ctrl, double* __restrict__ arc,
                                           uint8_t* __restrict__ feasible, double* s_fr) {
    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    const LdsFrames fr{s_fr + lane};
    const int D = T.D;
    cbody_t bodies = (cbody_t)T.bodies;
    cjoint_t joints = (cjoint_t)T.joints;
    ccgeom_t geoms = (ccgeom_t)T.geoms;
    bool blocked = static_mask != 0;
    if (WORLDS) {
        const unsigned qi = blockIdx.x / B;  // (< 64: the launch has at most 64 queries)
        bodies += (size_t)qi * T.nd;
        joints += (size_t)qi * nj;
        geoms += (size_t)qi * T.ng;
        blocked = ((static_mask >> qi) & 1ull) != 0;
    }
    for (int base = 0; base <= W && !blocked; base += kChainBlock) {
        const int i = base + lane;
        int h = 0;
        if (i <= W) {
            const double* N = tab + (size_t)i * (P + 1);
            double Nr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) Nr[r] = r <= P ? N[r] : 0.0;
            const double* c0 = ctrl + (size_t)b * n * D + (size_t)(span[i] - P) * D;
            // eval_pt's products and fma order for coordinate adr
            auto qv = [&](int adr) {
                double acc = Nr[0] * c0[adr];
#pragma unroll
                for (int r = 1; r <= 3; ++r)
                    if (r <= P) acc = fma(Nr[r], c0[r * D + adr], acc);
                return acc;
            };
            chain_fk(bodies, joints, T.nd, D, qv, fr);
            h = chain_contact(geoms, (ccpair_t)T.pairs, T.np, fr);
        }
        blocked = __any(h) != 0;  // wave-uniform: every lane leaves the loop together
    }
    if (lane == 0) {
        feasible[b] = blocked ? 0 : 1;
        if (blocked) arc[b] = INFINITY;
    }
}

__global__ __launch_bounds__(kChainBlock) void k_chain_feas(const ChainT T, const int static_block, const int P,
                                                             const int n, const int W,
                                                             const double* __restrict__ tab,
                                                             const int* __restrict__ span,
                                                             const double* __restrict__ ctrl,
                                                             double* __restrict__ arc,
                                                             uint8_t* __restrict__ feasible) {
    extern __shared__ double s_fr[];
    chain_feas<false>(T, static_block != 0, 0, 1, P, n, W, tab, span, ctrl, arc, feasible, s_fr);
}

// the worlds form: a batch of Q * B candidates, query q's in [q B, (q + 1) B); nj: joint records per world
__global__ __launch_bounds__(kChainBlock) void k_chain_feas_w(const ChainT T, const unsigned long long static_mask,
                                                               const int nj, const unsigned B, const int P,
                                                               const int n, const int W,
                                                               const double* __restrict__ tab,
                                                               const int* __restrict__ span,
                                                               const double* __restrict__ ctrl,
                                                               double* __restrict__ arc,
                                                               uint8_t* __restrict__ feasible) {
    extern __shared__ double s_fr[];
    chain_feas<true>(T, static_mask, nj, B, P, n, W, tab, span, ctrl, arc, feasible, s_fr);
}

// findBestPath per row q of arc / feasible [Q][B], one workgroup each: the (arc, id) minimum over
// the feasible candidates and their count, then the whole workgroup copies the winner's nd = n * D
// doubles from ctrl [Q][B][nd] to best_ctrl [Q][nd] (zeros without a winner), lanes on consecutive
// words.  out and best_ctrl are nullable (a single query: one workgroup, no best_ctrl) and may be
// mapped pinned host memory (plain stores, each word once).
constexpr int kBestBlock = 256;
__global__ __launch_bounds__(kBestBlock) void k_chain_best_q(const double* __restrict__ arc,
                                                              const uint8_t* __restrict__ feasible,
                                                              const double* __restrict__ ctrl, const long long B,
                                                              const long long first_id, const int nd,
                                                              sspp_best* __restrict__ out,
                                                              double* __restrict__ best_ctrl) {
    __shared__ double s_c[kBestBlock];
    __shared__ long long s_i[kBestBlock], s_n[kBestBlock];
    const long long q = blockIdx.x;
    const double* qa = arc + q * B;
    const uint8_t* qf = feasible + q * B;
    double bc = INFINITY;
    long long bi = -1, cnt = 0;
    for (long long k = threadIdx.x; k < B; k += kBestBlock) {
        if (!qf[k]) continue;
        ++cnt;
        const double a = qa[k];
        if (a < bc) { bc = a; bi = k; }  // (ascending k per thread: the lowest id of equal arcs stays)
    }
    s_c[threadIdx.x] = bc; s_i[threadIdx.x] = bi; s_n[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = kBestBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double oc = s_c[threadIdx.x + s];
            const long long oi = s_i[threadIdx.x + s];
            if (oi >= 0 && (s_i[threadIdx.x] < 0 || oc < s_c[threadIdx.x] ||
                            (oc == s_c[threadIdx.x] && oi < s_i[threadIdx.x]))) {
                s_c[threadIdx.x] = oc;
                s_i[threadIdx.x] = oi;
            }
            s_n[threadIdx.x] += s_n[threadIdx.x + s];
        }
        __syncthreads();
    }
    const long long win = s_i[0];  // (uniform: the loop's last barrier is behind every thread)
    if (best_ctrl) {
        const double* src = ctrl + ((size_t)q * (size_t)B + (size_t)(win >= 0 ? win : 0)) * (size_t)nd;
        double* dst = best_ctrl + (size_t)q * (size_t)nd;
        for (int t = threadIdx.x; t < nd; t += kBestBlock) dst[t] = win >= 0 ? src[t] : 0.0;
    }
    if (threadIdx.x == 0 && out) {
        out[q].cost = win >= 0 ? s_c[0] : INFINITY;
        out[q].index = win >= 0 ? first_id + win : -1;
        out[q].count = s_n[0];
        out[q].reserved = 0;
    }
}

}  // namespace sspc

extern "C" int sspp_chain_create(const sspp_model* m, int dof, int count_static, sspp_chain** out) {
    sspp::clear_error();
    if (!m || !out) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_create: null argument");
    if ((int)m->body_jnt_adr.size() != m->nbody())
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_create: the model has no joint tables");
    auto* c = new sspp_chain();
    int rc = chain_build(*m, dof, c->t);
    c->count_static = count_static;
    if (!rc) (void)hipGetDevice(&c->device);
    if (rc || (rc = c->d_bodies.upload(c->t.bodies.data(), c->t.bodies.size())) ||
        (rc = c->d_joints.upload(c->t.joints.data(), c->t.joints.size())) ||
        (rc = c->d_geoms.upload(c->t.geoms.data(), c->t.geoms.size())) ||
        (rc = c->d_pairs.upload(c->t.pairs.data(), c->t.pairs.size())) || (rc = c->d_jobbest.reserve(kChainMaxQueries))) {
        delete c;
        return rc;
    }
    c->model = *m;  // (the updates edit this copy: the caller's model is never touched)
    c->world = m->qpos0;
    *out = c;
    return SSPP_OK;
}

extern "C" void sspp_chain_free(sspp_chain* c) { delete c; }

// ---------------------------------------------------------------- worlds (DESIGN.md §5 "Worlds for arms")
// The chain to the world of (trial, world): a copy of its model data with new body_pos / body_quat,
// and a validated qpos.  The builder that created the chain runs first, so nothing is touched on a
// failure; then the device is drained and the tables are copied into the allocations they have.
static int chain_repose(sspp_chain* c, sspp_model&& trial, std::vector<double>&& world) {
    ChainTables t;
    if (int rc = chain_update(c->t, trial, world, t)) return rc;
    HIPCHK(hipDeviceSynchronize());
    if (!t.bodies.empty())
        HIPCHK(hipMemcpy(c->d_bodies.p, t.bodies.data(), sizeof(CBody) * t.bodies.size(), hipMemcpyHostToDevice));
    if (!t.joints.empty())
        HIPCHK(hipMemcpy(c->d_joints.p, t.joints.data(), sizeof(CJoint) * t.joints.size(), hipMemcpyHostToDevice));
    if (!t.geoms.empty())
        HIPCHK(hipMemcpy(c->d_geoms.p, t.geoms.data(), sizeof(CGeom) * t.geoms.size(), hipMemcpyHostToDevice));
    c->t = std::move(t);
    c->model = std::move(trial);
    c->world = std::move(world);
    ++c->epoch;
    return SSPP_OK;
}

extern "C" int sspp_chain_set_qpos(sspp_chain* c, const double* qpos, int nq) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_set_qpos: null chain");
    std::vector<double> world;
    if (int rc = chain_world_qpos(c->model, qpos, nq, "sspp_chain_set_qpos", world)) return rc;
    return chain_repose(c, sspp_model(c->model), std::move(world));
}

extern "C" int sspp_chain_set_body_pose(sspp_chain* c, int body, const double pos[3], const double quat[4]) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_set_body_pose: null chain");
    sspp_model trial(c->model);
    std::vector<double> world(c->world);
    if (int rc = chain_world_body_pose(trial, world, body, pos, quat)) return rc;
    return chain_repose(c, std::move(trial), std::move(world));
}

extern "C" int sspp_chain_get_qpos(const sspp_chain* c, double* qpos_out, int nq) {
    sspp::clear_error();
    if (!c || !qpos_out) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_get_qpos: null argument");
    if (nq != (int)c->world.size())
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_get_qpos: nq = " + std::to_string(nq) + ", the model has " +
                                                 std::to_string(c->world.size()));
    if (nq) std::memcpy(qpos_out, c->world.data(), sizeof(double) * nq);
    return SSPP_OK;
}

extern "C" int sspp_chain_epoch(const sspp_chain* c, int64_t* epoch) {
    sspp::clear_error();
    if (!c || !epoch) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_epoch: null argument");
    *epoch = c->epoch;
    return SSPP_OK;
}

extern "C" int sspp_chain_get_info(const sspp_chain* c, sspp_chain_info* out) {
    if (!c || !out) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_get_info: null argument");
    out->dof = c->t.D;
    out->n_driven_bodies = (int)c->t.bodies.size();
    out->n_geoms = (int)c->t.geoms.size();
    out->n_moving_geoms = c->t.n_moving_geoms;
    out->n_static_geoms = c->t.n_static_geoms;
    out->n_pairs = (int)c->t.pairs.size();
    out->n_static_pairs = c->t.n_static_pairs;
    out->static_contacts = c->t.static_contacts;
    return SSPP_OK;
}

extern "C" int sspp_chain_pairs(const sspp_chain* c, sspp_pair_info* out, int cap, int* n) {
    sspp::clear_error();
    if (!c || !n) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_pairs: null argument");
    *n = (int)c->t.pairs.size();
    if (!out) return SSPP_OK;
    if (cap < *n)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_pairs: cap = " + std::to_string(cap) + " < " +
                                                 std::to_string(*n) + " pairs");
    for (int k = 0; k < *n; ++k) {
        const CPair& p = c->t.pairs[k];
        const int g1 = std::min(p.a, p.b), g2 = std::max(p.a, p.b);
        out[k] = sspp_pair_info{g1, g2, c->t.geoms[g1].slot >= 0, c->t.geoms[g2].slot >= 0, p.margin};
    }
    return SSPP_OK;
}

extern "C" int sspp_chain_fk(const sspp_chain* c, const double* d_q, int64_t N, double* d_gpos, double* d_gmat,
                             void* stream) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_fk: null chain");
    if (N < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_fk: negative pose count");
    if (N == 0 || c->t.geoms.empty()) return SSPP_OK;
    if (!d_q || !d_gpos || !d_gmat) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_fk: null poses / output");
    int nblk = 0;
    if (int rc = chain_blocks(N, "sspp_chain", &nblk)) return rc;
    const ChainT T = c->view();
    hipLaunchKernelGGL(k_chain_fk, dim3(nblk), dim3(kChainBlock), chain_lds(T.nd), (hipStream_t)stream, T, d_q,
                       (long long)N, d_gpos, d_gmat);
    return sspo::hip_fail(hipGetLastError(), "sspp_chain_fk launch");
}

extern "C" int sspp_chain_contacts(const sspp_chain* c, const double* d_q, int64_t N, uint8_t* d_hit, void* stream) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_contacts: null chain");
    if (N < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_contacts: negative pose count");
    if (N == 0) return SSPP_OK;
    if (!d_q || !d_hit) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_contacts: null poses / output");
    int nblk = 0;
    if (int rc = chain_blocks(N, "sspp_chain", &nblk)) return rc;
    const ChainT T = c->view();
    hipLaunchKernelGGL(k_chain_contacts, dim3(nblk), dim3(kChainBlock), chain_lds(T.nd), (hipStream_t)stream, T,
                       c->static_block(), d_q, (long long)N, d_hit);
    return sspo::hip_fail(hipGetLastError(), "sspp_chain_contacts launch");
}

// the scene-less job for splines of this shape (created or replaced on a new shape or a larger
// batch: synchronous; otherwise nothing is allocated)
int sspc::chain_job(sspp_chain* c, const double* knots, int degree, int n, int W, int64_t B) {
    const int D = c->t.D;
    if (!knots) return sspp::set_error(SSPP_E_INVAL, "sspp_chain: null knots");
    if (degree < 2 || degree > 3 || n < degree + 1)
        return sspp::set_error(degree < 2 || degree > 3 ? SSPP_E_UNSUPPORTED : SSPP_E_INVAL,
                               "sspp_chain: spline degree 2 or 3 with at least degree + 1 control points");
    const size_t nk = (size_t)n + degree + 1;
    if (c->job && c->job_p == degree && c->job_n == n && c->job_W == W && c->job_cap >= B &&
        c->job_knots.size() == nk && std::memcmp(c->job_knots.data(), knots, sizeof(double) * nk) == 0)
        return SSPP_OK;
    if (c->job) {
        (void)hipDeviceSynchronize();  // (a launch may still read the older job's tables)
        sspp_job_free(c->job);
        c->job = nullptr;
    }
    const std::vector<double> zeros((size_t)n * D, 0.0), ones((size_t)D, 1.0);
    sspp_sspp_args a{};
    a.knots = knots; a.degree = degree; a.init_ctrl = zeros.data(); a.n_ctrl = n; a.dof = D;
    a.sigma = 0.0; a.limits = ones.data(); a.check_points = W; a.seed = 0; a.arc_all = 1;
    const int64_t cap = std::max<int64_t>(B, 1024);
    int rc = sspp_job_create_sspp(nullptr, &a, cap, &c->job);
    if (rc) return rc;
    c->job_knots.assign(knots, knots + nk);
    c->job_p = degree; c->job_n = n; c->job_W = W; c->job_cap = cap;
    return SSPP_OK;
}

// the device tables of a worlds launch's Q worlds and the queries' static blocks (bit q: query q)
struct WorldTables {
    const CBody* bodies;
    const CJoint* joints;
    const CGeom* geoms;
    int nj;
    unsigned long long static_mask;
};

// The tables of Q worlds (the chain's current world with its qpos replaced by worlds[q], host
// [Q][nq]) onto the device, stream-ordered.  Every world is validated and built first: a failure
// stages nothing.  The pinned staging and the device arrays are allocated once, for
// kChainMaxQueries worlds; the staging is rewritten after the event behind the previous set's copies.
static int chain_stage_worlds(sspp_chain* c, const char* who, int Q, const double* worlds, hipStream_t st,
                              WorldTables* out) {
    const int nq = (int)c->world.size();
    const size_t nd = c->t.bodies.size(), nj = c->t.joints.size(), ng = c->t.geoms.size();
    std::vector<CBody> hb;
    std::vector<CJoint> hj;
    std::vector<CGeom> hg;
    std::vector<double> w;
    ChainTables t;
    unsigned long long mask = 0;
    int rc;
    for (int q = 0; q < Q; ++q) {
        if ((rc = chain_world_qpos(c->model, worlds + (size_t)q * nq, nq, who, w)) ||
            (rc = chain_update(c->t, c->model, w, t)))
            return sspp::set_error(rc, "world " + std::to_string(q) + ": " + sspp_last_error());
        hb.insert(hb.end(), t.bodies.begin(), t.bodies.end());
        hj.insert(hj.end(), t.joints.begin(), t.joints.end());
        hg.insert(hg.end(), t.geoms.begin(), t.geoms.end());
        if (c->count_static && t.static_contacts > 0) mask |= 1ull << q;
    }
    const size_t cap = kChainMaxQueries;
    const auto up16 = [](size_t x) { return (x + 15) / 16 * 16; };
    const size_t oj = up16(sizeof(CBody) * cap * nd), og = oj + up16(sizeof(CJoint) * cap * nj);
    const size_t total = og + up16(sizeof(CGeom) * cap * ng);
    if ((rc = c->wst.wait())) return rc;
    if (!c->dw_bodies.p && !c->dw_joints.p && !c->dw_geoms.p) {  // the first worlds launch of this chain
        if ((rc = c->dw_bodies.reserve(cap * nd)) || (rc = c->dw_joints.reserve(cap * nj)) ||
            (rc = c->dw_geoms.reserve(cap * ng)) || (rc = c->wst.reserve(std::max<size_t>(total, 16))))
            return rc;
    }
    unsigned char* hp = c->wst.buf.p;
    if (nd) {
        std::memcpy(hp, hb.data(), sizeof(CBody) * hb.size());
        HIPCHK(hipMemcpyAsync(c->dw_bodies.p, hp, sizeof(CBody) * hb.size(), hipMemcpyHostToDevice, st));
    }
    if (nj) {
        std::memcpy(hp + oj, hj.data(), sizeof(CJoint) * hj.size());
        HIPCHK(hipMemcpyAsync(c->dw_joints.p, hp + oj, sizeof(CJoint) * hj.size(), hipMemcpyHostToDevice, st));
    }
    if (ng) {
        std::memcpy(hp + og, hg.data(), sizeof(CGeom) * hg.size());
        HIPCHK(hipMemcpyAsync(c->dw_geoms.p, hp + og, sizeof(CGeom) * hg.size(), hipMemcpyHostToDevice, st));
    }
    if ((rc = c->wst.record(st))) return rc;
    *out = WorldTables{c->dw_bodies.p, c->dw_joints.p, c->dw_geoms.p, (int)nj, mask};
    return SSPP_OK;
}

// feasibility of the Q * B candidates in d_ctrl ([Q][B][n][D]) over the job's arcs, then the argmin
// per row of B and, with d_best_ctrl, the winners' rows (many: a query launch, in a failure's
// message; wt: a worlds launch's tables, query q's candidates in world q)
static int chain_finish(sspp_chain* c, const double* d_ctrl, int64_t first_id, int Q, int64_t B, double* d_arc,
                        uint8_t* d_feasible, sspp_best* d_best, double* d_best_ctrl, bool many, hipStream_t st,
                        const WorldTables* wt = nullptr) {
    if (B > 0x7fffffffll)  // (a query launch has checked Q * B)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain: too many candidates for one launch");
    ChainT T = c->view();
    const sspp_job* j = c->job;
    if (wt) {
        T.bodies = wt->bodies; T.joints = wt->joints; T.geoms = wt->geoms;
        hipLaunchKernelGGL(k_chain_feas_w, dim3((int)(Q * B)), dim3(kChainBlock), chain_lds(T.nd), st, T, wt->static_mask,
                           wt->nj, (unsigned)B, j->p, j->n, j->W, j->d_tab.p, j->d_span.p, d_ctrl, d_arc, d_feasible);
    } else
        hipLaunchKernelGGL(k_chain_feas, dim3((int)(Q * B)), dim3(kChainBlock), chain_lds(T.nd), st, T, c->static_block(),
                           j->p, j->n, j->W, j->d_tab.p, j->d_span.p, d_ctrl, d_arc, d_feasible);
    if (int rc = sspo::hip_fail(hipGetLastError(), many ? "k_chain_feas query launch" : "k_chain_feas launch")) return rc;
    if (!d_best && !d_best_ctrl) return SSPP_OK;
    hipLaunchKernelGGL(k_chain_best_q, dim3(Q), dim3(kBestBlock), 0, st, d_arc, d_feasible, d_ctrl, (long long)B,
                       (long long)first_id, j->n * T.D, d_best, d_best_ctrl);
    return sspo::hip_fail(hipGetLastError(), many ? "k_chain_best_q launch" : "k_chain_best launch");
}

extern "C" int sspp_chain_score_ctrl(sspp_chain* c, const double* knots, int degree, const double* d_ctrl,
                                     int64_t first_id, int64_t B, int n, int W, double* d_arc, uint8_t* d_feasible,
                                     sspp_best* d_best, void* stream) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_score_ctrl: null chain");
    if (B < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_score_ctrl: negative batch");
    if (B == 0) return SSPP_OK;
    if (!d_ctrl || !d_arc || !d_feasible) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_score_ctrl: null argument");
    int rc;
    if ((rc = chain_job(c, knots, degree, n, W, B)) ||
        (rc = sspp_job_score_ctrl(c->job, d_ctrl, first_id, B, d_arc, d_feasible, c->d_jobbest.p, stream)))
        return rc;
    return chain_finish(c, d_ctrl, first_id, 1, B, d_arc, d_feasible, d_best, nullptr, false, (hipStream_t)stream);
}

extern "C" int sspp_chain_sample_score(sspp_chain* c, const double* knots, int degree, const double* init_ctrl, int n,
                                       int W, double sigma, const double* limits, uint64_t seed, int64_t first_id,
                                       int64_t B, double* d_arc, uint8_t* d_feasible, double* d_ctrl_out,
                                       sspp_best* d_best, void* stream) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_sample_score: null chain");
    if (B < 0) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_sample_score: negative batch");
    if (B == 0) return SSPP_OK;
    if (!init_ctrl || !limits || !d_arc || !d_feasible)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_sample_score: null argument");
    int rc;
    if ((rc = chain_job(c, knots, degree, n, W, B))) return rc;
    if (!d_ctrl_out) {  // the feasibility kernel reads the candidates: keep them in the chain's buffer
        if ((rc = c->d_ctrl.reserve((size_t)c->job_cap * n * c->t.D))) return rc;
        d_ctrl_out = c->d_ctrl.p;
    }
    if ((rc = sspp_job_update_sspp(c->job, init_ctrl, sigma, limits, seed, stream)) ||
        (rc = sspp_job_sample_score(c->job, first_id, B, d_arc, d_feasible, d_ctrl_out, c->d_jobbest.p, stream)))
        return rc;
    return chain_finish(c, d_ctrl_out, first_id, 1, B, d_arc, d_feasible, d_best, nullptr, false, (hipStream_t)stream);
}

// Q queries in one launch sequence (DESIGN.md §5 "Query launches for arms"): the scene-less job's
// query launch samples every query's candidates and writes their arcs ([Q][B], a batch of Q * B to
// the feasibility kernel), then one k_chain_best_q workgroup per query.  The job's single-query
// state, and with it what sspp_chain_sample_score writes, stays as it was.
// (worlds: null, or a worlds launch's [Q][nq]: query q's candidates meet world q)
static int chain_queries(sspp_chain* c, const std::string& who, const double* knots, int degree, int Q,
                         const double* init_ctrl, int n, int W, const double* sigma, const double* limits,
                         const uint64_t* seed, int64_t first_id, int64_t B, double* d_arc, uint8_t* d_feasible,
                         double* d_ctrl_out, sspp_best* d_best, double* d_best_ctrl, void* stream, bool with_worlds,
                         const double* worlds) {
    sspp::clear_error();
    if (!c) return sspp::set_error(SSPP_E_INVAL, who + ": null chain");
    if (Q < 1 || Q > kChainMaxQueries) return sspp::set_error(SSPP_E_INVAL, who + ": 1..64 queries, got " + std::to_string(Q));
    if (B < 0) return sspp::set_error(SSPP_E_INVAL, who + ": negative batch");
    if (B == 0) return SSPP_OK;
    if (!init_ctrl || !sigma || !limits || !seed || !d_arc || !d_feasible || (with_worlds && !worlds))
        return sspp::set_error(SSPP_E_INVAL, who + ": null argument");
    if (B > 0x7fffffffll / Q) return sspp::set_error(SSPP_E_INVAL, who + ": too many candidates for one launch");
    int rc;
    if ((rc = chain_job(c, knots, degree, n, W, B))) return rc;
    WorldTables wt{};
    if (with_worlds && (rc = chain_stage_worlds(c, who.c_str(), Q, worlds, (hipStream_t)stream, &wt))) return rc;
    if (!d_ctrl_out) {  // the feasibility kernel and the winner gather read the candidates
        const size_t need = (size_t)Q * (size_t)B * n * c->t.D;
        if (need > c->d_qctrl.n) {
            (void)hipDeviceSynchronize();  // (an earlier launch may still read the smaller buffer)
            if ((rc = c->d_qctrl.reserve(need))) return rc;
        }
        d_ctrl_out = c->d_qctrl.p;
    }
    if ((rc = sspp_job_set_queries(c->job, Q, init_ctrl, sigma, limits, seed, stream)) ||
        (rc = sspp_job_sample_score_queries(c->job, first_id, B, d_arc, d_feasible, d_ctrl_out, c->d_jobbest.p, stream)))
        return rc;
    return chain_finish(c, d_ctrl_out, first_id, Q, B, d_arc, d_feasible, d_best, d_best_ctrl, true, (hipStream_t)stream,
                        with_worlds ? &wt : nullptr);
}

extern "C" int sspp_chain_sample_score_queries(sspp_chain* c, const double* knots, int degree, int Q,
                                               const double* init_ctrl, int n, int W, const double* sigma,
                                               const double* limits, const uint64_t* seed, int64_t first_id,
                                               int64_t B, double* d_arc, uint8_t* d_feasible, double* d_ctrl_out,
                                               sspp_best* d_best, double* d_best_ctrl, void* stream) {
    return chain_queries(c, "sspp_chain_sample_score_queries", knots, degree, Q, init_ctrl, n, W, sigma, limits, seed,
                         first_id, B, d_arc, d_feasible, d_ctrl_out, d_best, d_best_ctrl, stream, false, nullptr);
}

extern "C" int sspp_chain_sample_score_worlds(sspp_chain* c, const double* knots, int degree, int Q,
                                              const double* init_ctrl, int n, int W, const double* sigma,
                                              const double* limits, const uint64_t* seed, int64_t first_id, int64_t B,
                                              double* d_arc, uint8_t* d_feasible, double* d_ctrl_out, sspp_best* d_best,
                                              double* d_best_ctrl, void* stream, const double* worlds) {
    return chain_queries(c, "sspp_chain_sample_score_worlds", knots, degree, Q, init_ctrl, n, W, sigma, limits, seed,
                         first_id, B, d_arc, d_feasible, d_ctrl_out, d_best, d_best_ctrl, stream, true, worlds);
}

// ---- the same on host buffers (the drop-in planner of an articulated model): staged to the device,
// run by the calls above and copied back on the drop-in planners' shared stream, which alone is waited for
extern "C" int sspp_chain_contacts_host(const sspp_chain* c, const double* q, int64_t N, uint8_t* hit) {
    sspp::clear_error();
    if (!c || !q || !hit || N < 1) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_contacts_host: bad argument");
    hipStream_t st = (hipStream_t)sspp::shared_stream(0);
    const size_t nq = (size_t)N * c->t.D;
    Dev<double> d_q;
    Dev<uint8_t> d_h;
    int rc;
    if ((rc = d_q.reserve(nq)) || (rc = d_h.reserve((size_t)N))) return rc;
    rc = hip_fail(hipMemcpyAsync(d_q.p, q, sizeof(double) * nq, hipMemcpyHostToDevice, st), "copy poses");
    if (!rc) rc = sspp_chain_contacts(c, d_q.p, N, d_h.p, st);
    if (!rc) rc = hip_fail(hipMemcpyAsync(hit, d_h.p, (size_t)N, hipMemcpyDeviceToHost, st), "copy hits");
    return chain_wait(st, rc, "sspp_chain_contacts_host");
}

static int chain_read_back(hipStream_t st, int rc, int64_t B, const Dev<double>& d_arc, const Dev<uint8_t>& d_f,
                           const Dev<sspp_best>& d_b, double* arc_out, uint8_t* feasible_out, sspp_best* best_out) {
    if (!rc && arc_out) rc = hip_fail(hipMemcpyAsync(arc_out, d_arc.p, sizeof(double) * B, hipMemcpyDeviceToHost, st), "copy arc");
    if (!rc && feasible_out) rc = hip_fail(hipMemcpyAsync(feasible_out, d_f.p, (size_t)B, hipMemcpyDeviceToHost, st), "copy feasible");
    if (!rc && best_out) rc = hip_fail(hipMemcpyAsync(best_out, d_b.p, sizeof(sspp_best), hipMemcpyDeviceToHost, st), "copy best");
    return chain_wait(st, rc, "sspp_chain host call");
}

extern "C" int sspp_chain_score_ctrl_host(sspp_chain* c, const double* knots, int degree, const double* ctrl, int64_t B,
                                          int n, int W, int with_collision, double* arc_out, uint8_t* feasible_out,
                                          sspp_best* best_out) {
    sspp::clear_error();
    if (!c || !knots || !ctrl || B < 1) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_score_ctrl_host: bad argument");
    hipStream_t st = (hipStream_t)sspp::shared_stream(0);
    const size_t nc = (size_t)B * n * c->t.D;
    Dev<double> d_ctrl, d_arc;
    Dev<uint8_t> d_f;
    Dev<sspp_best> d_b;
    int rc;
    if ((rc = d_ctrl.reserve(nc)) || (rc = d_arc.reserve((size_t)B)) || (rc = d_f.reserve((size_t)B)) ||
        (rc = d_b.reserve(1)))
        return rc;
    rc = hip_fail(hipMemcpyAsync(d_ctrl.p, ctrl, sizeof(double) * nc, hipMemcpyHostToDevice, st), "copy splines");
    if (!rc && with_collision) rc = sspp_chain_score_ctrl(c, knots, degree, d_ctrl.p, 0, B, n, W, d_arc.p, d_f.p, d_b.p, st);
    if (!rc && !with_collision && !(rc = chain_job(c, knots, degree, n, W, B)))
        rc = sspp_job_score_ctrl(c->job, d_ctrl.p, 0, B, d_arc.p, d_f.p, d_b.p, st);
    return chain_read_back(st, rc, B, d_arc, d_f, d_b, arc_out, feasible_out, best_out);
}

extern "C" int sspp_chain_plan_host(sspp_chain* c, const double* start, const double* end, double sigma,
                                    const double* limits, int sample_count, int check_points, int init_points,
                                    uint64_t seed, double* knots_out, double* ctrl_out, uint8_t* feasible_out,
                                    double* arc_out, sspp_best* best_out) {
    sspp::clear_error();
    if (!c || !start || !end || !limits || !knots_out)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_plan_host: null argument");
    const int n = init_points, D = c->t.D, deg = 3;
    if (sample_count < 1) return sspp::set_error(SSPP_E_INVAL, "sample_count must be >= 1");
    if (n < deg + 1) return sspp::set_error(SSPP_E_INVAL, "init_points must be >= 4 for a cubic spline");
    if (check_points < 2) return sspp::set_error(SSPP_E_INVAL, "check_points must be >= 2");
    std::vector<double> ctrl0((size_t)n * D);
    int rc;
    if ((rc = sspp::initialize_path(start, end, n, D, deg, knots_out, ctrl0.data()))) return rc;
    hipStream_t st = (hipStream_t)sspp::shared_stream(0);
    const int64_t B = sample_count;
    const size_t nc = (size_t)B * n * D;
    Dev<double> d_ctrl, d_arc;
    Dev<uint8_t> d_f;
    Dev<sspp_best> d_b;
    if ((rc = d_ctrl.reserve(nc)) || (rc = d_arc.reserve((size_t)B)) || (rc = d_f.reserve((size_t)B)) ||
        (rc = d_b.reserve(1)))
        return rc;
    rc = sspp_chain_sample_score(c, knots_out, deg, ctrl0.data(), n, check_points, sigma, limits, seed, 0, B, d_arc.p,
                                 d_f.p, d_ctrl.p, d_b.p, st);
    if (!rc && ctrl_out) rc = hip_fail(hipMemcpyAsync(ctrl_out, d_ctrl.p, sizeof(double) * nc, hipMemcpyDeviceToHost, st), "copy candidates");
    return chain_read_back(st, rc, B, d_arc, d_f, d_b, arc_out, feasible_out, best_out);
}

// device bytes of one chunk's candidates: larger sets go in chunks of fewer queries (sspp_planner_plan_many's cap)
constexpr size_t kChainManyCtrlBytes = (size_t)256 << 20;

// SamplingPathPlanner::plan for Q queries of one arm: initializePath per query on the host, then per
// chunk of at most kChainMaxQueries queries one sspp_chain_sample_score_queries whose k_chain_best_q
// writes the records and the winners' rows straight into the chain's mapped pinned memory (Q rows;
// no candidate leaves the device), one stream synchronisation at the end.
// (worlds: null, or [Q][nq]: sspp_chain_plan_many_worlds_host, every world validated before the first chunk)
static int chain_plan_many(sspp_chain* c, int Q, const double* starts, const double* ends, double sigma,
                           const double* limits, int sample_count, int check_points, int init_points,
                           const uint64_t* seeds, int64_t first_id, double* knots_out, sspp_best* best_out,
                           double* best_ctrl_out, int64_t* n_feasible, double* arc_out, uint8_t* feasible_out,
                           bool with_worlds, const double* worlds) {
    sspp::clear_error();
    if (!c || !starts || !ends || !limits || !seeds || !knots_out || !best_out || !best_ctrl_out || !n_feasible ||
        (with_worlds && !worlds))
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_plan_many_host: null argument");
    if (Q < 1) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_plan_many_host: Q must be >= 1");
    const int n = init_points, D = c->t.D, deg = 3;
    if (sample_count < 1) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_plan_many_host: sample_count must be >= 1");
    if (n < deg + 1)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_plan_many_host: init_points must be >= 4 for a cubic spline");
    if (check_points < 2) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_plan_many_host: check_points must be >= 2");
    // initializePath per query; the knot vector depends on n only
    const size_t nd = (size_t)n * D, nq = c->world.size();
    const int64_t B = sample_count;
    std::vector<double> ctrl0((size_t)Q * nd);
    int rc;
    if (with_worlds) {  // (a bad world in a later chunk must not leave earlier chunks launched)
        std::vector<double> w;
        for (int q = 0; q < Q; ++q)
            if ((rc = chain_world_qpos(c->model, worlds + (size_t)q * nq, (int)nq, "sspp_chain_plan_many_worlds_host", w)))
                return sspp::set_error(rc, "world " + std::to_string(q) + ": " + sspp_last_error());
    }
    for (int q = 0; q < Q; ++q)
        if ((rc = sspp::initialize_path(starts + (size_t)q * D, ends + (size_t)q * D, n, D, deg, knots_out,
                                        ctrl0.data() + q * nd)))
            return rc;
    const int chunk = (int)std::min<size_t>(kChainMaxQueries,
                                            std::max<size_t>(1, kChainManyCtrlBytes / (sizeof(double) * (size_t)B * nd)));
    const int qc_max = std::min(Q, chunk);
    hipStream_t st = (hipStream_t)sspp::shared_stream(0);
    if ((rc = c->dm_arc.reserve((size_t)qc_max * B)) || (rc = c->dm_feas.reserve((size_t)qc_max * B)) ||
        (rc = c->hm_best.reserve((size_t)Q)) || (rc = c->hm_ctrl.reserve((size_t)Q * nd)) ||
        (arc_out && (rc = c->hm_arc.reserve((size_t)Q * B))) || (feasible_out && (rc = c->hm_feas.reserve((size_t)Q * B))))
        return rc;
    sspp_best* hb = c->hm_best.dev();
    double* hc = c->hm_ctrl.dev();
    if (!hb || !hc) return sspp::set_error(SSPP_E_HIP, "hipHostGetDevicePointer failed");
    std::vector<double> sig((size_t)qc_max, sigma), lim((size_t)qc_max * D);
    for (int q = 0; q < qc_max; ++q) std::memcpy(lim.data() + (size_t)q * D, limits, sizeof(double) * D);
    rc = SSPP_OK;
    for (int q0 = 0; q0 < Q && !rc; q0 += chunk) {
        const int qc = std::min(chunk, Q - q0);
        rc = chain_queries(c, with_worlds ? "sspp_chain_sample_score_worlds" : "sspp_chain_sample_score_queries", knots_out,
                           deg, qc, ctrl0.data() + (size_t)q0 * nd, n, check_points, sig.data(), lim.data(), seeds + q0,
                           first_id, B, c->dm_arc.p, c->dm_feas.p, nullptr, hb + q0, hc + (size_t)q0 * nd, st, with_worlds,
                           with_worlds ? worlds + (size_t)q0 * nq : nullptr);
        if (!rc && arc_out)
            rc = hip_fail(hipMemcpyAsync(c->hm_arc.p + (size_t)q0 * B, c->dm_arc.p, sizeof(double) * qc * B,
                                         hipMemcpyDeviceToHost, st), "copy arc");
        if (!rc && feasible_out)
            rc = hip_fail(hipMemcpyAsync(c->hm_feas.p + (size_t)q0 * B, c->dm_feas.p, (size_t)qc * B,
                                         hipMemcpyDeviceToHost, st), "copy feasible");
    }
    const std::string why = rc ? sspp_last_error() : "";
    const int rs = hip_fail(hipStreamSynchronize(st), "sspp_chain_plan_many_host");  // (also after a failure: work is queued)
    if (rc) return sspp::set_error(rc, why);
    if (rs) return rs;
    if ((rc = sspp_best_check(c->hm_best.p, Q))) return rc;
    std::memcpy(best_out, c->hm_best.p, sizeof(sspp_best) * Q);
    std::memcpy(best_ctrl_out, c->hm_ctrl.p, sizeof(double) * Q * nd);
    for (int q = 0; q < Q; ++q) n_feasible[q] = best_out[q].count;
    if (arc_out) std::memcpy(arc_out, c->hm_arc.p, sizeof(double) * Q * B);
    if (feasible_out) std::memcpy(feasible_out, c->hm_feas.p, (size_t)Q * B);
    return SSPP_OK;
}

extern "C" int sspp_chain_plan_many_host(sspp_chain* c, int Q, const double* starts, const double* ends, double sigma,
                                         const double* limits, int sample_count, int check_points, int init_points,
                                         const uint64_t* seeds, int64_t first_id, double* knots_out,
                                         sspp_best* best_out, double* best_ctrl_out, int64_t* n_feasible,
                                         double* arc_out, uint8_t* feasible_out) {
    return chain_plan_many(c, Q, starts, ends, sigma, limits, sample_count, check_points, init_points, seeds, first_id,
                           knots_out, best_out, best_ctrl_out, n_feasible, arc_out, feasible_out, false, nullptr);
}

extern "C" int sspp_chain_plan_many_worlds_host(sspp_chain* c, int Q, const double* starts, const double* ends,
                                                double sigma, const double* limits, int sample_count, int check_points,
                                                int init_points, const uint64_t* seeds, int64_t first_id,
                                                double* knots_out, sspp_best* best_out, double* best_ctrl_out,
                                                int64_t* n_feasible, double* arc_out, uint8_t* feasible_out,
                                                const double* worlds) {
    return chain_plan_many(c, Q, starts, ends, sigma, limits, sample_count, check_points, init_points, seeds, first_id,
                           knots_out, best_out, best_ctrl_out, n_feasible, arc_out, feasible_out, true, worlds);
}
