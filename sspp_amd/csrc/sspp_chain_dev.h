// sspp_chain_dev.h — what the chain's two translation units share (sspp_chain.hip: kinematics,
// contact decisions, scoring; sspp_chain_report.hip: the contact report): the device view of the
// tables, the LDS-backed frame accessor, the launches' block count and the _host calls' tail, the
// chain object and its per-shape job cache.
#pragma once
#include "sspp_chain.h"

namespace sspc {

constexpr int kChainBlock = 64;  // one wave: the frames' LDS is per lane, nothing is shared
constexpr int kChainMaxQueries = 64;  // queries of one query launch (sspp_job_set_queries' limit)

struct ChainT {
    const CBody* __restrict__ bodies;
    const CJoint* __restrict__ joints;
    const CGeom* __restrict__ geoms;
    const CPair* __restrict__ pairs;
    int nd, ng, np, D;
};

struct LdsFrames {
    double* base;  // + lane
    __device__ __forceinline__ double get(int slot, int c) const { return base[(slot * 7 + c) * kChainBlock]; }
    __device__ __forceinline__ void set(int slot, int c, double v) const { base[(slot * 7 + c) * kChainBlock] = v; }
};

inline size_t chain_lds(int nd) { return sizeof(double) * 7 * kChainBlock * (size_t)std::max(1, nd); }

// workgroups of kChainBlock lanes for a launch over items poses
inline int chain_blocks(int64_t items, const char* who, int* out) {
    const int64_t nblk = (items + kChainBlock - 1) / kChainBlock;
    if (nblk > 0x7fffffffll) return sspp::set_error(SSPP_E_INVAL, std::string(who) + ": too many poses for one launch");
    *out = (int)nblk;
    return SSPP_OK;
}

// the tail of a _host call: its stream is waited for also after a failure (work is queued on it, and
// the staged input and the outputs die with the caller's frame)
inline int chain_wait(hipStream_t st, int rc, const char* what) {
    const int rs = sspo::hip_fail(hipStreamSynchronize(st), what);
    return rc ? rc : rs;
}

}  // namespace sspc

struct sspp_chain {
    sspc::ChainTables t;
    int count_static = 0;
    int device = 0;
    sspo::Dev<sspc::CBody> d_bodies;
    sspo::Dev<sspc::CJoint> d_joints;
    sspo::Dev<sspc::CGeom> d_geoms;
    sspo::Dev<sspc::CPair> d_pairs;
    // the scene-less job of the last spline shape (arc lengths, sampled candidates, the report's
    // basis rows), the candidates of a sample_score call without d_ctrl_out, and the job's own
    // argmin record (not the chain's)
    sspp_job* job = nullptr;
    std::vector<double> job_knots;
    int job_p = 0, job_n = 0, job_W = 0;
    int64_t job_cap = 0;
    sspo::Dev<double> d_ctrl;
    sspo::Dev<sspp_best> d_jobbest;  // kChainMaxQueries records: a query launch's job writes one per query
    // query launches (sspp_chain_sample_score_queries): the candidates [Q][B][n][D] of a launch
    // without d_ctrl_out.  sspp_chain_plan_many_host: one chunk's device outputs, and the whole
    // call's results in pinned memory (records and winner rows mapped: k_chain_best_q writes them)
    sspo::Dev<double> d_qctrl;
    sspo::Dev<double> dm_arc;
    sspo::Dev<uint8_t> dm_feas;
    sspo::Pinned<sspp_best> hm_best{hipHostMallocMapped | hipHostMallocCoherent};
    sspo::Pinned<double> hm_ctrl{hipHostMallocMapped | hipHostMallocCoherent};
    sspo::Pinned<double> hm_arc;
    sspo::Pinned<uint8_t> hm_feas;
    // worlds (DESIGN.md §5 "Worlds for arms"): the chain's own copy of the model data, which the
    // updates edit, and its world's qpos (model.qpos0 stays every joint's zero).  A worlds launch:
    // the Q worlds' body, joint and geom records, staged in pinned memory (bodies | joints | geoms,
    // each at a 16-byte boundary) and copied into device arrays [Q][nd], [Q][nj], [Q][ng]
    sspp_model model;
    std::vector<double> world;
    int64_t epoch = 0;
    sspo::Staging wst;
    sspo::Dev<sspc::CBody> dw_bodies;
    sspo::Dev<sspc::CJoint> dw_joints;
    sspo::Dev<sspc::CGeom> dw_geoms;
    ~sspp_chain() {
        if (job) sspp_job_free(job);
    }
    int static_block() const { return (count_static && t.static_contacts > 0) ? 1 : 0; }
    sspc::ChainT view() const {
        return sspc::ChainT{d_bodies.p, d_joints.p, d_geoms.p, d_pairs.p, (int)t.bodies.size(), (int)t.geoms.size(),
                            (int)t.pairs.size(), t.D};
    }
};

namespace sspc {
// the scene-less job for splines of this shape (created or replaced on a new shape or a larger
// batch: synchronous; otherwise nothing is allocated).  Defined in sspp_chain.hip.
int chain_job(sspp_chain* c, const double* knots, int degree, int n, int W, int64_t B);
}  // namespace sspc
