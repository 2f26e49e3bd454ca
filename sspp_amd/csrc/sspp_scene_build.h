// sspp_scene_build.h — a scene's host tables from (model data with its poses, mode, moving bodies).
//
// sspp_scene_create and the scene updates (sspp_scene_set_qpos, sspp_scene_set_body_pose) both go
// through scene_build, so a re-posed scene holds what a scene created from a model with the new
// poses holds by construction.  Host only: no device call (tests/scene_update
// builds it without a GPU).
#pragma once
#include <cassert>

#include "sspp_kern.h"

namespace sspb {

// MuJoCo-like kinematics on the host (same operation order as oracle/sspp_oracle.c::fk)
inline void host_fk(const sspp_model& m, const std::vector<double>& qpos, std::vector<double>& xpos,
                    std::vector<double>& xquat, std::vector<double>& xmat, std::vector<double>& gxpos,
                    std::vector<double>& gxmat) {
    int nb = m.nbody(), ng = m.ngeom();
    xpos.assign(3 * nb, 0.0); xquat.assign(4 * nb, 0.0); xmat.assign(9 * nb, 0.0);
    gxpos.assign(3 * ng, 0.0); gxmat.assign(9 * ng, 0.0);
    xquat[0] = 1.0;
    quat2mat(&xquat[0], &xmat[0]);
    for (int b = 1; b < nb; ++b) {
        double* p = &xpos[3 * b];
        double* q = &xquat[4 * b];
        if (m.body_jnt_type[b] == 0) {
            const double* qp = &qpos[m.body_qpos_adr[b]];
            p[0] = qp[0]; p[1] = qp[1]; p[2] = qp[2];
            q[0] = qp[3]; q[1] = qp[4]; q[2] = qp[5]; q[3] = qp[6];
        } else {
            int pa = m.body_parent[b];
            double t[3];
            matvec3(&xmat[9 * pa], &m.body_pos[3 * b], t);
            p[0] = xpos[3 * pa] + t[0]; p[1] = xpos[3 * pa + 1] + t[1]; p[2] = xpos[3 * pa + 2] + t[2];
            mulquat(&xquat[4 * pa], &m.body_quat[4 * b], q);
        }
        normalize4(q);
        quat2mat(q, &xmat[9 * b]);
    }
    for (int g = 0; g < ng; ++g) {
        int b = m.geom_body[g];
        double t[3], gq[4];
        matvec3(&xmat[9 * b], &m.geom_pos[3 * g], t);
        gxpos[3 * g] = xpos[3 * b] + t[0];
        gxpos[3 * g + 1] = xpos[3 * b + 1] + t[1];
        gxpos[3 * g + 2] = xpos[3 * b + 2] + t[2];
        mulquat(&xquat[4 * b], &m.geom_quat[4 * g], gq);
        normalize4(gq);
        quat2mat(gq, &gxmat[9 * g]);
    }
}

// everything a scene derives on the host from its model's poses
struct SceneTables {
    std::vector<DGeom> geoms;
    std::vector<DPair> pairs, visit;  // visit: the pairs grouped by moving geom (SceneT::visit)
    std::vector<DMover> movers;
    int n_moving_geoms = 0, n_static_geoms = 0, n_static_pairs = 0, static_contacts = 0;
    double static_cost = 0.0;
    std::vector<StaticPair> statics;  // the n_static_pairs env-env pairs, (g1, g2) order
};

// The tables of model m (poses: its qpos0 / body_pos / body_quat) for the moving bodies
// mover_bodies of a scene of `mode`.  SSPP_E_UNSUPPORTED (message set) for a pair the
// narrowphase does not cover; out is then unspecified.
inline int scene_build(const sspp_model& mdl, int mode, const std::vector<int>& mover_bodies, SceneTables& out) {
    const sspp_model* m = &mdl;
    SceneTables* s = &out;
    *s = SceneTables();
    const int nb = m->nbody(), ng = m->ngeom();
    std::vector<int> weld(nb, 0), moving(nb, 0), mover_of(nb, -1);
    for (int b = 1; b < nb; ++b)
        weld[b] = (m->body_jnt_type[b] != -1) ? b : weld[m->body_parent[b]];
    for (size_t i = 0; i < mover_bodies.size(); ++i) {
        moving[mover_bodies[i]] = 1;
        mover_of[mover_bodies[i]] = (int)i;
    }
    // kinematics at qpos0: world poses of static geoms
    std::vector<double> xpos, xquat, xmat, gxpos, gxmat;
    host_fk(*m, m->qpos0, xpos, xquat, xmat, gxpos, gxmat);
    // moving geoms relative to their mover root: same FK with every mover at the identity
    std::vector<double> qrel = m->qpos0;
    for (int b : mover_bodies) {
        int adr = m->body_qpos_adr[b];
        double id[7] = {0, 0, 0, 1, 0, 0, 0};
        for (int k = 0; k < 7; ++k) qrel[adr + k] = id[k];
    }
    std::vector<double> rxpos, rxquat, rxmat, rgxpos, rgxmat;
    host_fk(*m, qrel, rxpos, rxquat, rxmat, rgxpos, rgxmat);

    std::vector<int> table_index(ng, -1);
    for (int g = 0; g < ng; ++g) {
        int b = m->geom_body[g];
        int w = weld[b];
        bool mv = moving[w];
        DGeom dg{};
        dg.type = m->geom_type[g];
        dg.mover = mv ? mover_of[w] : -1;
        dg.orig = g;
        const std::vector<double>& P = mv ? rgxpos : gxpos;
        const std::vector<double>& M = mv ? rgxmat : gxmat;
        for (int k = 0; k < 3; ++k) dg.pos[k] = P[3 * g + k];
        for (int k = 0; k < 9; ++k) dg.mat[k] = M[9 * g + k];
        for (int k = 0; k < 3; ++k) dg.size[k] = m->geom_size[3 * g + k];
        dg.rbound = geom_rbound(dg.type, dg.size);
        dg.relrot = 0;
        for (int k = 0; k < 9; ++k) dg.relrot |= dg.mat[k] != ((k % 4 == 0) ? 1.0 : 0.0);
        dg.reach = mv ? std::sqrt(dg.pos[0] * dg.pos[0] + dg.pos[1] * dg.pos[1] + dg.pos[2] * dg.pos[2]) * (1.0 + 1e-12)
                      : 0.0;
        fill_f32(dg);
        table_index[g] = (int)s->geoms.size();
        s->geoms.push_back(dg);
        if (m->geom_contype[g] || m->geom_conaffinity[g]) {
            if (mv) s->n_moving_geoms++; else s->n_static_geoms++;
        }
    }
    // mj_collision pair filter, (g1 < g2) order
    struct P2 { int g1, g2; double margin; bool stat; };
    std::vector<P2> all;
    for (int g1 = 0; g1 < ng; ++g1) {
        for (int g2 = g1 + 1; g2 < ng; ++g2) {
            int b1 = m->geom_body[g1], b2 = m->geom_body[g2];
            int w1 = weld[b1], w2 = weld[b2];
            if (w1 == w2) continue;
            int ct1 = m->geom_contype[g1], ca1 = m->geom_conaffinity[g1];
            int ct2 = m->geom_contype[g2], ca2 = m->geom_conaffinity[g2];
            if (!((ct1 & ca2) || (ct2 & ca1))) continue;
            if (w1 != 0 && w2 != 0 &&
                (w1 == weld[m->body_parent[w2]] || w2 == weld[m->body_parent[w1]]))
                continue;
            bool excl = false;
            for (size_t e = 0; e + 1 < m->exclude.size(); e += 2) {
                int e1 = m->exclude[e], e2 = m->exclude[e + 1];
                if ((e1 == b1 && e2 == b2) || (e1 == b2 && e2 == b1)) { excl = true; break; }
            }
            if (excl) continue;
            if (!pair_supported(m->geom_type[g1], m->geom_type[g2]))
                return sspp::set_error(SSPP_E_UNSUPPORTED,
                                       "unsupported collision pair: geom '" + m->geom_names[g1] +
                                           "' (type " + std::to_string(m->geom_type[g1]) + ") vs '" +
                                           m->geom_names[g2] + "' (type " +
                                           std::to_string(m->geom_type[g2]) + ")");
            double mg = std::max(m->geom_margin[g1], m->geom_margin[g2]);
            all.push_back({g1, g2, mg, !(moving[w1] || moving[w2])});
        }
    }
    // env-env pairs: constant over waypoints -> evaluated once here (same device math)
    for (auto& pr : all) {
        if (!pr.stat) continue;
        s->n_static_pairs++;
        s->statics.push_back({pr.g1, pr.g2, pr.margin, 0, 0});
        const DGeom& A = s->geoms[table_index[pr.g1]];
        const DGeom& B = s->geoms[table_index[pr.g2]];
        double dc[3] = {B.pos[0] - A.pos[0], B.pos[1] - A.pos[1], B.pos[2] - A.pos[2]};
        if (A.rbound > 0.0 && B.rbound > 0.0) {
            double thr = A.rbound + B.rbound + pr.margin;
            if (dot3(dc, dc) > thr * thr) continue;
        }
        bool afirst = A.type <= B.type;
        const DGeom& F = afirst ? A : B;
        const DGeom& S = afirst ? B : A;
        int nd = 0;
        int nc = collide<false>(F.type, F.pos, F.mat, F.size, S.type, S.pos, S.mat, S.size, pr.margin, &nd);
        collide<true>(F.type, F.pos, F.mat, F.size, S.type, S.pos, S.mat, S.size, pr.margin, &nd);
        s->static_contacts += nc;
        s->statics.back().contact = (uint8_t)nc;
        s->statics.back().deep = (uint8_t)nd;
        if (nd > 0) {
            double term = -1.0 / (sqrt(dot3(dc, dc)) + 1e-4);
            for (int i = 0; i < nd; ++i) s->static_cost = s->static_cost + term;
        }
    }
    // moving pairs: sspp mode groups by moving geom (pose computed once per group);
    // tsp mode keeps the oracle's (g1, g2) order so per-waypoint cost sums match bit for bit.
    std::vector<P2> mov;
    for (auto& pr : all)
        if (!pr.stat) mov.push_back(pr);
    auto moving_geom = [&](const P2& pr) {
        int w1 = weld[m->geom_body[pr.g1]];
        return moving[w1] ? pr.g1 : pr.g2;
    };
    if (mode == SSPP_MODE_QPOS) {
        std::stable_sort(mov.begin(), mov.end(), [&](const P2& x, const P2& y) {
            return moving_geom(x) < moving_geom(y);
        });
    }
    for (auto& pr : mov) {
        int gm = moving_geom(pr);
        int go = gm == pr.g1 ? pr.g2 : pr.g1;
        DPair dp{};
        dp.gm = table_index[gm];
        dp.go = table_index[go];
        const DGeom& O = s->geoms[dp.go];
        dp.otype = O.type;
        dp.oorig = O.orig;
        dp.omover = O.mover;
        dp.margin = pr.margin;
        for (int k = 0; k < 3; ++k) dp.opos[k] = O.pos[k];
        for (int k = 0; k < 9; ++k) dp.omat[k] = O.mat[k];
        for (int k = 0; k < 3; ++k) dp.osize[k] = O.size[k];
        dp.orbound = O.rbound;
        fill_f32(dp);
        s->pairs.push_back(dp);
    }
    for (size_t i = 0; i < mover_bodies.size(); ++i) {
        DMover mv{};
        mv.qpos_adr = m->body_qpos_adr[mover_bodies[i]];
        for (int k = 0; k < 7; ++k) mv.qpos0[k] = m->qpos0[mv.qpos_adr + k];
        s->movers.push_back(mv);
    }
    // the pair visit order of the record-form pair loops (SceneT::visit): grouped by moving geom,
    // the reference's order within a group; only for tables a mask word can cover
    if (!s->pairs.empty() && s->pairs.size() <= 64) {
        std::vector<int> ix(s->pairs.size());
        for (size_t i = 0; i < ix.size(); ++i) ix[i] = (int)i;
        std::stable_sort(ix.begin(), ix.end(), [&](int x, int y) { return s->pairs[x].gm < s->pairs[y].gm; });
        for (int i : ix) {
            DPair q = s->pairs[i];
            q.pad = i;  // its record index
            s->visit.push_back(q);
        }
    }
    return SSPP_OK;
}

// An update's new poses into a copy of the scene's model data, validated: SSPP_E_INVAL (message
// set) leaves `m` untouched.  Quaternions are normalised as the loader does (sspp::loader_normq).
inline bool pose_values_ok(const double* v, int n, const double* quat) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return quat[0] != 0.0 || quat[1] != 0.0 || quat[2] != 0.0 || quat[3] != 0.0;
}
inline int model_set_qpos(sspp_model& m, const double* qpos, int nq) {
    if (!qpos) return sspp::set_error(SSPP_E_INVAL, "sspp_scene_set_qpos: null qpos");
    if (nq != (int)m.qpos0.size())
        return sspp::set_error(SSPP_E_INVAL, "sspp_scene_set_qpos: nq = " + std::to_string(nq) + ", the model has " +
                                                 std::to_string(m.qpos0.size()));
    for (int a = 0; a + 7 <= nq; a += 7)
        if (!pose_values_ok(qpos + a, 7, qpos + a + 3))
            return sspp::set_error(SSPP_E_INVAL, "sspp_scene_set_qpos: non-finite value or zero quaternion at qpos[" +
                                                     std::to_string(a) + ":" + std::to_string(a + 7) + "]");
    m.qpos0.assign(qpos, qpos + nq);
    for (int a = 0; a + 7 <= nq; a += 7) sspp::loader_normq(&m.qpos0[a + 3]);
    return SSPP_OK;
}
inline int model_set_body_pose(sspp_model& m, int body, const double* pos, const double* quat) {
    if (!pos || !quat) return sspp::set_error(SSPP_E_INVAL, "sspp_scene_set_body_pose: null pos / quat");
    if (body < 1 || body >= m.nbody())
        return sspp::set_error(SSPP_E_INVAL, "sspp_scene_set_body_pose: body id " + std::to_string(body) +
                                                 " out of range [1, " + std::to_string(m.nbody()) + ")");
    if (!pose_values_ok(pos, 3, quat) || !pose_values_ok(quat, 4, quat))
        return sspp::set_error(SSPP_E_INVAL, "sspp_scene_set_body_pose: non-finite value or zero quaternion");
    double q[4] = {quat[0], quat[1], quat[2], quat[3]};
    sspp::loader_normq(q);
    // a free body's pose lives in qpos0 (the loader leaves the same values in body_pos / body_quat,
    // which the kinematics never read for it); a jointless body's is relative to its parent
    for (int k = 0; k < 3; ++k) m.body_pos[3 * body + k] = pos[k];
    for (int k = 0; k < 4; ++k) m.body_quat[4 * body + k] = q[k];
    if (m.body_jnt_type[body] == 0) {
        const int a = m.body_qpos_adr[body];
        for (int k = 0; k < 3; ++k) m.qpos0[a + k] = pos[k];
        for (int k = 0; k < 4; ++k) m.qpos0[a + 3 + k] = q[k];
    }
    return SSPP_OK;
}

}  // namespace sspb
