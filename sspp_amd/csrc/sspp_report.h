// sspp_report.h — the contact report's per-pose routine (DESIGN.md §5 "Contact report").
//
// One pose against every moving pair of a scene's pair table: per pair, `contact` = what
// sspd::collide<false> returns (the count behind SamplingPathPlanner's ncon > 0, include/sspp.h:139-147)
// and `deep` = collide<true>'s *nd (contacts with dist < -1e-3, the multiplicity of Collision.h's
// cost terms, include/Collision.h:84-103).  The reference reads the same from mjData's contact[]
// (Collision::check_collision_point, include/Collision.h:51-82).
//
// The routine is __host__ __device__: the kernels of sspp_report.hip are thin loops around it, and
// tests/contact_report/check_report.cpp runs the same code on the CPU.  It restates point_collide's
// pose arithmetic call for call (mover_poses, geom_pos_t / geom_rot_t, the partner's pose of a
// mover-mover pair, pair_near, geom 1 first by (type, model index)), without any early exit, mask
// or reordering: column k is pair k of the scene's table, whatever a job scans.
#pragma once
#include "sspp_kern.h"

namespace sspr {

using namespace sspd;
using namespace sspk;

// The collider forms a scene's scoring kernels take (sspk::kscene, tsp_dispatch), so that the report
// and the scores come from the same code:
//   kGeneric  the exact cylinder-box / cylinder-cylinder tests beside the capsule colliders and the
//             generic box-box manifold (every SamplingPathPlanner scene; TaskSpacePlanner scenes
//             with a capsule pair or a tilted cylinder / box: point_collide's CB = 1)
//   kVertical every cylinder-box and cylinder-cylinder pair is vertical / upright (host-checked):
//             their closed forms only (CB = 2 / 3; a scene without such pairs takes it too, as CB = 0
//             does: the compiled-out code is never reached)
//   kUpright  kVertical with every box-box pair upright (UP)
enum { kGeneric = 0, kVertical = 1, kUpright = 2 };

inline int form_of(const KScene& sc) {
    const int cbm = sc.cylbox ? (sc.cbup ? 2 : 1) : 0;
    if (cbm == 1) return kGeneric;
    return sc.upright ? kUpright : kVertical;
}

template <bool DEEP, int FORM>
SSPP_HD int collide_form(int t1, const double* p1, const double* m1, const double* s1, int t2, const double* p2,
                         const double* m2, const double* s2, double margin, int* nd) {
    constexpr int CB = FORM == kGeneric ? 1 : 2;
    return collide<DEEP, CB, DEEP, false, FORM == kUpright, FORM == kGeneric, false, CB>(t1, p1, m1, s1, t2, p2, m2, s2,
                                                                                        margin, nd);
}

// Mover poses of one pose q: MODE 0 reads the qpos window [0, D) (entries past it: the scene's
// defaults), the selection mover_poses<D, NM, 0> makes at compile time; MODE 1 is mover_poses itself.
// q holds kPoseVals<NM, MODE> readable values (the callers gather a pose into registers, entries
// past D unspecified), so every index below is a compile-time constant.
template <int NM, int MODE>
constexpr int kPoseVals = MODE == 1 ? 4 : 7 * NM;
// gather pose row `src` of D values into q[kPoseVals]
template <int NM, int MODE>
SSPP_HD void gather_pose(const double* src, int D, double (&q)[kPoseVals<NM, MODE>]) {
#pragma unroll
    for (int k = 0; k < kPoseVals<NM, MODE>; ++k) q[k] = k < D ? src[k] : 0.0;
}
template <int NM, int MODE>
SSPP_HD void poses_of(const double* q, int D, cmover_t movers, double (&mp)[NM][3], double (&mR)[NM][9]) {
    if (MODE == 1) {
        mover_poses<4, NM, 1>(q, movers, mp, mR);
        return;
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        double qp[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) qp[k] = (7 * m + k < D) ? q[7 * m + k] : (double)movers[m].qpos0[k];
        normalize4(qp + 3);
        quat2mat(qp + 3, mR[m]);
        mp[m][0] = qp[0]; mp[m][1] = qp[1]; mp[m][2] = qp[2];
    }
}

// One pose against pairs [0, np): contact[k] and (when non-null) deep[k] for every k, zeros included.
template <int NM, int MODE, int FORM>
SSPP_HD void pose_report(const double* q, int D, cgeom_t geoms, cpair_t pairs, cmover_t movers, int np,
                         uint8_t* contact, uint8_t* deep) {
    constexpr bool ZR = MODE == 1;  // yaw-only mover rotation
    double mp[NM][3], mR[NM][9];
    poses_of<NM, MODE>(q, D, movers, mp, mR);
    int cur = -1;
    double gp[3], gmat[9];
    DGeom G;
    for (int k = 0; k < np; ++k) {
        const DPair pr = load_pair(pairs + k);
        if (pr.gm != cur) {
            cur = pr.gm;
            G = load_geom(geoms + cur);
            const bool second = NM > 1 && G.mover == 1;
            geom_pos_t<ZR>(second ? mp[NM - 1] : mp[0], second ? mR[NM - 1] : mR[0], G, gp);
            geom_rot_t<ZR>(second ? mR[NM - 1] : mR[0], G, gmat);
        }
        double op_[3], om_[9];
        const double* op = pr.opos;
        const double* om = pr.omat;
        if (NM > 1 && pr.omover >= 0) {
            const bool second = pr.omover == 1;
            const double* R = second ? mR[NM - 1] : mR[0];
            const double* P = second ? mp[NM - 1] : mp[0];
            double t[3];
            matvec3(R, pr.opos, t);
            op_[0] = P[0] + t[0]; op_[1] = P[1] + t[1]; op_[2] = P[2] + t[2];
            matmul3(R, pr.omat, om_);
            op = op_; om = om_;
        }
        int nc = 0, nd = 0;
        if (pair_near(pr, G.rbound, gp, op, om)) {
            const bool gfirst = (G.type < pr.otype) || (G.type == pr.otype && G.orig < pr.oorig);
            int unused = 0;
            if (gfirst) {
                nc = collide_form<false, FORM>(G.type, gp, gmat, G.size, pr.otype, op, om, pr.osize, pr.margin, &unused);
                if (deep) collide_form<true, FORM>(G.type, gp, gmat, G.size, pr.otype, op, om, pr.osize, pr.margin, &nd);
            } else {
                nc = collide_form<false, FORM>(pr.otype, op, om, pr.osize, G.type, gp, gmat, G.size, pr.margin, &unused);
                if (deep) collide_form<true, FORM>(pr.otype, op, om, pr.osize, G.type, gp, gmat, G.size, pr.margin, &nd);
            }
        }
        contact[k] = (uint8_t)nc;
        if (deep) deep[k] = (uint8_t)nd;
    }
}

// the routine for a scene's (mode, movers, form), on the host: f is called once with
// std::integral_constants (NM, MODE, FORM)
template <class F>
void dispatch_form(int mode, int nm, int form, F&& f) {
    auto pick_form = [&](auto nmc, auto modec) {
        if constexpr (decltype(modec)::value == 1) {
            if (form == kUpright) return f(nmc, modec, std::integral_constant<int, kUpright>{});
            if (form == kVertical) return f(nmc, modec, std::integral_constant<int, kVertical>{});
        }
        f(nmc, modec, std::integral_constant<int, kGeneric>{});
    };
    if (mode == SSPP_MODE_BODY) pick_form(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
    else if (nm > 1) pick_form(std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{});
    else pick_form(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
}

}  // namespace sspr
