// sspp_chain.h — articulated movers: hinge and slide joints (DESIGN.md §5 "Articulated movers").
//
// A chain is a model with hinge / slide joints (sspp_model_load_mjcf_joints) bound to
// SamplingPathPlanner's pose rule q[0:D] -> qpos[0:D].  This header holds everything that is a
// function of (model, D): the tables (chain_build) and, per pose, the forward kinematics of the
// driven bodies (chain_fk), a geom's world pose (geom_pose) and the contact decision over the pair
// table (chain_contact).  The per-pose routines are __host__ __device__: the kernels of
// sspp_chain.hip are thin loops around them, and tests/chain/check_chain.cpp runs the same code on
// the CPU.  The free-body path (sspp_scene, k_sspp_c2f) shares nothing with it but the colliders.
//
// Kinematics: MuJoCo's mj_kinematics, restated (and, like the colliders, MuJoCo-unpinned).  Bodies
// in index order, parents first.  A free body: its 7 qpos.  Any other body: xpos = xpos[parent] +
// R[parent] body_pos, xquat = xquat[parent] * body_quat; then per joint, in order, with the current
// xquat / xpos: anchor = xpos + R(xquat) jnt_pos, xaxis = R(xquat) jnt_axis; a slide adds
// xaxis (q - qpos0) to xpos; a hinge multiplies xquat by (cos(a/2), jnt_axis sin(a/2)), a = q - qpos0,
// and puts xpos at anchor - R(xquat) jnt_pos.  Finally xquat is normalised.  Geom poses from body
// poses as sspb::host_fk forms them.
//
// Worlds (DESIGN.md §5 "Worlds for arms"): what the pose rule does not drive comes from a world, a
// full qpos [nq] beside the model's body poses.  qpos0 stays every joint's zero; a frozen joint's
// value (CJoint::qf) and a frozen free body's (CBody::q0, components at or past D) are the world's.
// chain_build takes the world, so creation, re-posing and a query's own world are one builder.
//
// Frames are read and written through an accessor (get / set of (body slot, component 0..6: pos,
// quat)), and the pose's values through a functor of the qpos address, so that a kernel can keep its
// lanes' frames in LDS [slot][component][lane] and evaluate a spline's coordinate when a joint asks
// for it; nothing here indexes a per-lane array with a run-time index.
#pragma once
#include "sspp_report.h"

namespace sspc {

using namespace sspd;

constexpr int kMaxBodies = SSPP_CHAIN_MAX_BODIES;
constexpr int kMaxDof = SSPP_CHAIN_MAX_DOF;
constexpr int kMaxPairs = SSPP_CHAIN_MAX_PAIRS;

// sin and cos as the same IEEE operations on host and device (the tests compare bytes): a
// quarter-turn reduction k = rint(a 2/pi), r = a - k pi/2 in two fma steps (pi/2 split so that
// k * hi is exact for |k| < 2^20), then fma Horner polynomials on |r| <= pi/4 (the classic minimax
// coefficients, errors below 1 ulp), swapped and signed by k mod 4.
SSPP_HD void chain_sincos(double a, double* sn, double* cs) {
    const double k = rint(a * 0.63661977236758138);
    double r = fma(-k, 1.57079632673412561417e+00, a);
    r = fma(-k, 6.07710050650619224932e-11, r);
    const double z = r * r;
    double ps = 1.58969099521155010221e-10;
    ps = fma(ps, z, -2.50507602534068634195e-08);
    ps = fma(ps, z, 2.75573137070700676789e-06);
    ps = fma(ps, z, -1.98412698298579493134e-04);
    ps = fma(ps, z, 8.33333333332248946124e-03);
    ps = fma(ps, z, -1.66666666666666324348e-01);
    const double s = fma(r * z, ps, r);
    double pc = -1.13596475577881948265e-11;
    pc = fma(pc, z, 2.08757232129817482790e-09);
    pc = fma(pc, z, -2.75573143513906633035e-07);
    pc = fma(pc, z, 2.48015872894767294178e-05);
    pc = fma(pc, z, -1.38888888888741095749e-03);
    pc = fma(pc, z, 4.16666666666666019037e-02);
    const double c = fma(z * z, pc, fma(-0.5, z, 1.0));
    const int m = (int)((long long)k & 3);
    const double s1 = (m & 1) ? c : s, c1 = (m & 1) ? s : c;
    *sn = (m & 2) ? -s1 : s1;
    *cs = (m == 1 || m == 2) ? -c1 : c1;
}

// ---------------------------------------------------------------- tables
// a driven body, in model index order (parents first)
struct CBody {
    int32_t parent;    // slot of its parent among the driven bodies; -1: a static parent (ppos / pquat)
    int32_t free_adr;  // a free body's qpos address, -1 for any other body
    int32_t jnt0, njnt;  // its hinge / slide joints in the CJoint table
    double pos[3], quat[4];    // relative to the parent (mjModel.body_pos / body_quat)
    double ppos[3], pquat[4];  // a static parent's world pose
    double q0[7];              // a free body's frozen values: the world's at addresses >= D (qpos0 below)
};
struct CJoint {
    int32_t type;  // 2 slide, 3 hinge
    int32_t adr;   // qpos address below D, -1: frozen at qf
    double axis[3], pos[3], q0;  // q0: the joint's zero (qpos0)
    double qf;     // the world's value of a frozen joint (q0 for a driven one: never read)
};
// every geom of the model, model order
struct CGeom {
    int32_t type, slot;  // slot: its driven body, -1 static
    int32_t orig, pad;
    double pos[3], quat[4];   // relative to its body
    double wpos[3], wmat[9];  // a static geom's world pose
    double size[3], rbound;
};
// a pair in collide order: a first by (type, model index)
struct CPair {
    int32_t a, b;
    double margin;
};

#if defined(__HIP_DEVICE_COMPILE__)
#define SSPC_CONST __attribute__((address_space(4)))
#else
#define SSPC_CONST
#endif
typedef const SSPC_CONST CBody* cbody_t;
typedef const SSPC_CONST CJoint* cjoint_t;
typedef const SSPC_CONST CGeom* ccgeom_t;
typedef const SSPC_CONST CPair* ccpair_t;

// frames of one pose in a plain array [slot][7] (host; the kernels' accessor is LDS-backed)
struct ArrayFrames {
    double* f;
    SSPP_HD double get(int slot, int c) const { return f[slot * 7 + c]; }
    SSPP_HD void set(int slot, int c, double v) const { f[slot * 7 + c] = v; }
};

// ---------------------------------------------------------------- per pose
// Forward kinematics of the nd driven bodies: qv(adr) is the pose's value at qpos address adr < D.
// (the table pointers are template parameters: constant-address-space ones in a kernel, so that the
// records are scalar loads, plain ones on the host)
template <class BP, class JP, class QV, class FR>
SSPP_HD void chain_fk(BP bodies, JP joints, int nd, int D, const QV& qv, const FR& fr) {
    for (int s = 0; s < nd; ++s) {
        double p[3], q[4];
        const int fa = bodies[s].free_adr;
        if (fa >= 0) {
            double v[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) v[k] = (fa + k < D) ? qv(fa + k) : (double)bodies[s].q0[k];
            p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
            q[0] = v[3]; q[1] = v[4]; q[2] = v[5]; q[3] = v[6];
        } else {
            double pp[3], pq[4], bp[3], bq[4], R[9], t[3];
            const int par = bodies[s].parent;
            if (par >= 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) pp[k] = fr.get(par, k);
#pragma unroll
                for (int k = 0; k < 4; ++k) pq[k] = fr.get(par, 3 + k);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) pp[k] = bodies[s].ppos[k];
#pragma unroll
                for (int k = 0; k < 4; ++k) pq[k] = bodies[s].pquat[k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) bp[k] = bodies[s].pos[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) bq[k] = bodies[s].quat[k];
            quat2mat(pq, R);
            matvec3(R, bp, t);
            p[0] = pp[0] + t[0]; p[1] = pp[1] + t[1]; p[2] = pp[2] + t[2];
            mulquat(pq, bq, q);
            const int j0 = bodies[s].jnt0, j1 = j0 + bodies[s].njnt;
            for (int j = j0; j < j1; ++j) {
                const int adr = joints[j].adr;
                const double q0 = joints[j].q0;
                const double a = (adr >= 0 ? qv(adr) : (double)joints[j].qf) - q0;
                double ax[3], jp[3], xa[3], anchor[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) { ax[k] = joints[j].axis[k]; jp[k] = joints[j].pos[k]; }
                quat2mat(q, R);
                matvec3(R, jp, t);
                anchor[0] = p[0] + t[0]; anchor[1] = p[1] + t[1]; anchor[2] = p[2] + t[2];
                if (joints[j].type == SSPP_JNT_SLIDE) {
                    matvec3(R, ax, xa);
                    p[0] = fma(xa[0], a, p[0]); p[1] = fma(xa[1], a, p[1]); p[2] = fma(xa[2], a, p[2]);
                } else {
                    double sn, cs, qn[4];
                    chain_sincos(0.5 * a, &sn, &cs);
                    const double ql[4] = {cs, ax[0] * sn, ax[1] * sn, ax[2] * sn};
                    mulquat(q, ql, qn);
                    q[0] = qn[0]; q[1] = qn[1]; q[2] = qn[2]; q[3] = qn[3];
                    quat2mat(q, R);
                    matvec3(R, jp, t);
                    p[0] = anchor[0] - t[0]; p[1] = anchor[1] - t[1]; p[2] = anchor[2] - t[2];
                }
            }
        }
        normalize4(q);
#pragma unroll
        for (int k = 0; k < 3; ++k) fr.set(s, k, p[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) fr.set(s, 3 + k, q[k]);
    }
}

// world pose of geom g: position gp[3], rotation gm[9] (as sspb::host_fk forms a geom's)
template <class GP, class FR>
SSPP_HD void geom_pose(GP g, const FR& fr, double* gp, double* gm) {
    const int slot = g->slot;
    if (slot < 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) gp[k] = g->wpos[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) gm[k] = g->wmat[k];
        return;
    }
    double p[3], q[4], R[9], lp[3], lq[4], t[3], gq[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[k] = fr.get(slot, k); lp[k] = g->pos[k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { q[k] = fr.get(slot, 3 + k); lq[k] = g->quat[k]; }
    quat2mat(q, R);
    matvec3(R, lp, t);
    gp[0] = p[0] + t[0]; gp[1] = p[1] + t[1]; gp[2] = p[2] + t[2];
    mulquat(q, lq, gq);
    normalize4(gq);
    quat2mat(gq, gm);
}

// 1 iff some pair of [0, np) is in contact at the frames fr: the bounding-sphere test (planes never
// culled), then collide<false> in the generic form, geom a first.  The pair loop is wave-uniform
// (records are scalar loads, the type branch is uniform); a geom's pose is kept while consecutive
// pairs share it.  A lane that has its contact skips the colliders of the later pairs.
template <class GP, class PP, class FR>
SSPP_HD int chain_contact(GP geoms, PP pairs, int np, const FR& fr) {
    int cur1 = -1, cur2 = -1, hit = 0;
    double p1[3], m1[9], p2[3], m2[9];
    for (int k = 0; k < np; ++k) {
        const int a = pairs[k].a, b = pairs[k].b;
        const double margin = pairs[k].margin;
        if (a != cur1) { geom_pose(geoms + a, fr, p1, m1); cur1 = a; }
        if (b != cur2) { geom_pose(geoms + b, fr, p2, m2); cur2 = b; }
        if (hit) continue;
        const double r1 = geoms[a].rbound, r2 = geoms[b].rbound;
        if (r1 > 0.0 && r2 > 0.0) {
            const double dc[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
            const double thr = r1 + r2 + margin;
            if (dot3(dc, dc) > thr * thr) continue;
        }
        double s1[3], s2[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { s1[i] = geoms[a].size[i]; s2[i] = geoms[b].size[i]; }
        int unused = 0;
        const int nc = sspr::collide_form<false, sspr::kGeneric>(geoms[a].type, p1, m1, s1, geoms[b].type, p2, m2, s2,
                                                                 margin, &unused);
        hit = nc > 0;
    }
    return hit;
}

// ---------------------------------------------------------------- host: the tables of (model, D)
// a static-static pair, (geom1, geom2) order, with its counts at the static poses (the contact
// report's sspp_chain_static_pairs; the contact counts sum to static_contacts)
struct CStatic {
    int32_t g1, g2;
    double margin;
    uint8_t contact, deep;
};

// counts of one pair at world poses: the bounding-sphere cull (a zero rbound is never culled), then
// collide<false>'s count and collide<true>'s deep count in the generic form, geom F first.  The one
// test behind static_contacts and the static pairs' report.
inline void chain_static_counts(const CGeom& F, const CGeom& S, double margin, int* contact, int* deep) {
    *contact = *deep = 0;
    if (F.rbound > 0.0 && S.rbound > 0.0) {
        const double dc[3] = {S.wpos[0] - F.wpos[0], S.wpos[1] - F.wpos[1], S.wpos[2] - F.wpos[2]};
        const double thr = F.rbound + S.rbound + margin;
        if (dot3(dc, dc) > thr * thr) return;
    }
    int unused = 0;
    *contact = sspr::collide_form<false, sspr::kGeneric>(F.type, F.wpos, F.wmat, F.size, S.type, S.wpos, S.wmat, S.size,
                                                         margin, &unused);
    sspr::collide_form<true, sspr::kGeneric>(F.type, F.wpos, F.wmat, F.size, S.type, S.wpos, S.wmat, S.size, margin, deep);
}

struct ChainTables {
    int D = 0;
    std::vector<CBody> bodies;    // the driven bodies
    std::vector<CJoint> joints;   // their hinge / slide joints
    std::vector<CGeom> geoms;     // every geom
    std::vector<CPair> pairs;     // evaluated per pose, (geom1, geom2) order
    std::vector<CStatic> statics; // static-static pairs, (geom1, geom2) order, evaluated once
    std::vector<int> slot_body;   // model body of a slot
    int n_moving_geoms = 0, n_static_geoms = 0, n_static_pairs = 0, static_contacts = 0;
};

// body and joint records of the bodies with in[b] != 0 (closed under descendants), joints with a
// qpos address at or past D frozen at world's values (world: qpos [nq], chain_build's: qpos0 below
// its D); wframe: world frames [nbody][7] of the bodies outside the set
inline void chain_records(const sspp_model& m, int D, const double* world, const std::vector<int>& in,
                          const std::vector<double>& wframe, std::vector<CBody>& bodies, std::vector<CJoint>& joints,
                          std::vector<int>& slot_of) {
    const int nb = m.nbody();
    slot_of.assign(nb, -1);
    for (int b = 1; b < nb; ++b) {
        if (!in[b]) continue;
        CBody B{};
        const int pa = m.body_parent[b];
        B.parent = slot_of[pa];
        B.free_adr = m.body_jnt_type[b] == 0 ? m.body_qpos_adr[b] : -1;
        for (int k = 0; k < 3; ++k) B.pos[k] = m.body_pos[3 * b + k];
        for (int k = 0; k < 4; ++k) B.quat[k] = m.body_quat[4 * b + k];
        B.pquat[0] = 1.0;
        if (B.parent < 0 && !wframe.empty()) {
            for (int k = 0; k < 3; ++k) B.ppos[k] = wframe[7 * pa + k];
            for (int k = 0; k < 4; ++k) B.pquat[k] = wframe[7 * pa + 3 + k];
        }
        if (B.free_adr >= 0) {
            for (int k = 0; k < 7; ++k) B.q0[k] = world[B.free_adr + k];
        } else {
            B.jnt0 = (int)joints.size();
            for (int j = m.body_jnt_adr[b]; j < m.body_jnt_adr[b] + m.body_jnt_num[b]; ++j) {
                CJoint J{};
                J.type = m.jnt_type[j];
                J.adr = m.jnt_qpos_adr[j] < D ? m.jnt_qpos_adr[j] : -1;
                for (int k = 0; k < 3; ++k) { J.axis[k] = m.jnt_axis[3 * j + k]; J.pos[k] = m.jnt_pos[3 * j + k]; }
                J.q0 = m.qpos0[m.jnt_qpos_adr[j]];
                J.qf = world[m.jnt_qpos_adr[j]];
                joints.push_back(J);
            }
            B.njnt = (int)joints.size() - B.jnt0;
        }
        slot_of[b] = (int)bodies.size();
        bodies.push_back(B);
    }
}

// n finite values and, where given, a quaternion that is not zero (sspb::pose_values_ok's test)
inline bool world_values_ok(const double* v, int n, const double* quat) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return !quat || quat[0] != 0.0 || quat[1] != 0.0 || quat[2] != 0.0 || quat[3] != 0.0;
}

// A world's qpos, validated and normalised as the loader does, into out [nq]: SSPP_E_INVAL (message
// set, out untouched) for a wrong nq, a non-finite value or a free joint's zero quaternion.
inline int chain_world_qpos(const sspp_model& m, const double* qpos, int nq, const char* who, std::vector<double>& out) {
    if (!qpos) return sspp::set_error(SSPP_E_INVAL, std::string(who) + ": null qpos");
    if (nq != (int)m.qpos0.size())
        return sspp::set_error(SSPP_E_INVAL, std::string(who) + ": nq = " + std::to_string(nq) + ", the model has " +
                                                 std::to_string(m.qpos0.size()));
    for (int j = 0; j < m.njnt(); ++j) {
        const int a = m.jnt_qpos_adr[j], w = m.jnt_type[j] == 0 ? 7 : 1;
        if (!world_values_ok(qpos + a, w, w == 7 ? qpos + a + 3 : nullptr))
            return sspp::set_error(SSPP_E_INVAL, std::string(who) + ": non-finite value or zero quaternion at qpos[" +
                                                     std::to_string(a) + ":" + std::to_string(a + w) + "]");
    }
    out.assign(qpos, qpos + nq);
    for (int j = 0; j < m.njnt(); ++j)
        if (m.jnt_type[j] == 0) sspp::loader_normq(&out[m.jnt_qpos_adr[j] + 3]);
    return SSPP_OK;
}

// One body's new pose into model data m and world (sspp_chain_set_body_pose): a free-joint body's 7
// world values (and, as the loader leaves them, its body_pos / body_quat); any other body's pose
// relative to its parent.  SSPP_E_INVAL (message set) leaves both untouched.
inline int chain_world_body_pose(sspp_model& m, std::vector<double>& world, int body, const double* pos, const double* quat) {
    if (!pos || !quat) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_set_body_pose: null pos / quat");
    if (body < 1 || body >= m.nbody())
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_set_body_pose: body id " + std::to_string(body) +
                                                 " out of range [1, " + std::to_string(m.nbody()) + ")");
    if (!world_values_ok(pos, 3, nullptr) || !world_values_ok(quat, 4, quat))
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_set_body_pose: non-finite value or zero quaternion");
    double q[4] = {quat[0], quat[1], quat[2], quat[3]};
    sspp::loader_normq(q);
    for (int k = 0; k < 3; ++k) m.body_pos[3 * body + k] = pos[k];
    for (int k = 0; k < 4; ++k) m.body_quat[4 * body + k] = q[k];
    if (m.body_jnt_type[body] == 0) {
        const int a = m.body_qpos_adr[body];
        for (int k = 0; k < 3; ++k) world[a + k] = pos[k];
        for (int k = 0; k < 4; ++k) world[a + 3 + k] = q[k];
    }
    return SSPP_OK;
}

// The tables of model m for the pose rule q[0:D] -> qpos[0:D], the rest from world (qpos [nq],
// validated: chain_world_qpos; null: the model's own, qpos0).  SSPP_E_INVAL for D out of range,
// SSPP_E_UNSUPPORTED past a limit or for a pair the narrowphase does not cover (message set).
inline int chain_build(const sspp_model& m, int D, ChainTables& out, const double* world = nullptr) {
    out = ChainTables();
    // entries below D are the pose's: never read, so the tables hold qpos0 there in every world
    std::vector<double> held(m.qpos0);
    for (size_t a = (size_t)std::max(D, 0); world && a < held.size(); ++a) held[a] = world[a];
    world = held.data();
    const int nb = m.nbody(), ng = m.ngeom(), nq = (int)m.qpos0.size();
    if (D < 1) return sspp::set_error(SSPP_E_INVAL, "sspp_chain_create: dof must be >= 1");
    if (D > nq)
        return sspp::set_error(SSPP_E_INVAL, "sspp_chain_create: dof = " + std::to_string(D) + " > nq = " +
                                                 std::to_string(nq));
    if (D > kMaxDof)
        return sspp::set_error(SSPP_E_UNSUPPORTED, "sspp_chain_create: dof = " + std::to_string(D) +
                                                       " exceeds the limit of " + std::to_string(kMaxDof));
    out.D = D;
    // world frames of every body in the world: the same routine over all bodies with every joint frozen
    std::vector<double> wframe((size_t)7 * nb, 0.0);
    wframe[3] = 1.0;
    {
        std::vector<int> all(nb, 1), slot_of;
        std::vector<CBody> bodies;
        std::vector<CJoint> joints;
        chain_records(m, 0, world, all, std::vector<double>(), bodies, joints, slot_of);
        std::vector<double> f((size_t)7 * std::max(1, nb - 1));
        chain_fk(bodies.data(), joints.data(), (int)bodies.size(), 0, [](int) { return 0.0; }, ArrayFrames{f.data()});
        for (int b = 1; b < nb; ++b)
            for (int k = 0; k < 7; ++k) wframe[7 * b + k] = f[7 * slot_of[b] + k];
    }
    // driven: the body or an ancestor has a joint with a qpos address below D
    std::vector<int> driven(nb, 0), weld(nb, 0);
    for (int b = 1; b < nb; ++b) {
        driven[b] = driven[m.body_parent[b]];
        for (int j = m.body_jnt_adr[b]; j < m.body_jnt_adr[b] + m.body_jnt_num[b]; ++j)
            if (m.jnt_qpos_adr[j] < D) driven[b] = 1;
        weld[b] = m.body_jnt_num[b] > 0 ? b : weld[m.body_parent[b]];
    }
    std::vector<int> slot_of;
    chain_records(m, D, world, driven, wframe, out.bodies, out.joints, slot_of);
    if ((int)out.bodies.size() > kMaxBodies)
        return sspp::set_error(SSPP_E_UNSUPPORTED, "sspp_chain_create: " + std::to_string(out.bodies.size()) +
                                                       " driven bodies exceed the limit of " +
                                                       std::to_string(kMaxBodies));
    out.slot_body.assign(out.bodies.size(), 0);
    for (int b = 1; b < nb; ++b)
        if (slot_of[b] >= 0) out.slot_body[slot_of[b]] = b;
    // geoms: static ones posed once, here
    const ArrayFrames wf{wframe.data()};
    for (int g = 0; g < ng; ++g) {
        CGeom G{};
        const int b = m.geom_body[g];
        G.type = m.geom_type[g];
        G.slot = b;  // (posed from the world frames first)
        G.orig = g;
        for (int k = 0; k < 3; ++k) { G.pos[k] = m.geom_pos[3 * g + k]; G.size[k] = m.geom_size[3 * g + k]; }
        for (int k = 0; k < 4; ++k) G.quat[k] = m.geom_quat[4 * g + k];
        G.rbound = geom_rbound(G.type, G.size);
        double wp[3], wm[9];
        geom_pose(&G, wf, wp, wm);
        for (int k = 0; k < 3; ++k) G.wpos[k] = wp[k];
        for (int k = 0; k < 9; ++k) G.wmat[k] = wm[k];
        G.slot = slot_of[b];
        if (m.geom_contype[g] || m.geom_conaffinity[g]) {
            if (G.slot >= 0) out.n_moving_geoms++; else out.n_static_geoms++;
        }
        out.geoms.push_back(G);
    }
    // sspb::scene_build's pair filter, (g1 < g2) order
    for (int g1 = 0; g1 < ng; ++g1) {
        for (int g2 = g1 + 1; g2 < ng; ++g2) {
            const int b1 = m.geom_body[g1], b2 = m.geom_body[g2];
            const int w1 = weld[b1], w2 = weld[b2];
            if (w1 == w2) continue;
            const int ct1 = m.geom_contype[g1], ca1 = m.geom_conaffinity[g1];
            const int ct2 = m.geom_contype[g2], ca2 = m.geom_conaffinity[g2];
            if (!((ct1 & ca2) || (ct2 & ca1))) continue;
            if (w1 != 0 && w2 != 0 && (w1 == weld[m.body_parent[w2]] || w2 == weld[m.body_parent[w1]])) continue;
            bool excl = false;
            for (size_t e = 0; e + 1 < m.exclude.size(); e += 2) {
                const int e1 = m.exclude[e], e2 = m.exclude[e + 1];
                if ((e1 == b1 && e2 == b2) || (e1 == b2 && e2 == b1)) { excl = true; break; }
            }
            if (excl) continue;
            if (!pair_supported(m.geom_type[g1], m.geom_type[g2]))
                return sspp::set_error(SSPP_E_UNSUPPORTED,
                                       "unsupported collision pair: geom '" + m.geom_names[g1] + "' (type " +
                                           std::to_string(m.geom_type[g1]) + ") vs '" + m.geom_names[g2] +
                                           "' (type " + std::to_string(m.geom_type[g2]) + ")");
            const CGeom& A = out.geoms[g1];
            const CGeom& B = out.geoms[g2];
            const bool afirst = A.type <= B.type;
            CPair P{};
            P.a = afirst ? g1 : g2;
            P.b = afirst ? g2 : g1;
            P.margin = std::max(m.geom_margin[g1], m.geom_margin[g2]);
            if (A.slot >= 0 || B.slot >= 0) {
                out.pairs.push_back(P);
                continue;
            }
            // static-static: constant over poses, evaluated once (the per-pose test, its contact count
            // summed as sspb::scene_build sums static_contacts)
            out.n_static_pairs++;
            int nc = 0, nd = 0;
            chain_static_counts(out.geoms[P.a], out.geoms[P.b], P.margin, &nc, &nd);
            out.static_contacts += nc;
            out.statics.push_back(CStatic{g1, g2, P.margin, (uint8_t)nc, (uint8_t)nd});
        }
    }
    if ((int)out.pairs.size() > kMaxPairs)
        return sspp::set_error(SSPP_E_UNSUPPORTED, "sspp_chain_create: " + std::to_string(out.pairs.size()) +
                                                       " pairs exceed the limit of " + std::to_string(kMaxPairs));
    return SSPP_OK;
}

// what a world cannot change (the pair filter does not look at poses): the driven set, every
// table's length, the pair table and the bounding radii
inline bool chain_same_shape(const ChainTables& a, const ChainTables& b) {
    if (a.D != b.D || a.bodies.size() != b.bodies.size() || a.joints.size() != b.joints.size() ||
        a.geoms.size() != b.geoms.size() || a.pairs.size() != b.pairs.size() || a.statics.size() != b.statics.size() ||
        a.slot_body != b.slot_body || a.n_moving_geoms != b.n_moving_geoms || a.n_static_pairs != b.n_static_pairs)
        return false;
    for (size_t k = 0; k < a.pairs.size(); ++k)
        if (a.pairs[k].a != b.pairs[k].a || a.pairs[k].b != b.pairs[k].b || a.pairs[k].margin != b.pairs[k].margin)
            return false;
    for (size_t g = 0; g < a.geoms.size(); ++g)
        if (a.geoms[g].slot != b.geoms[g].slot || a.geoms[g].rbound != b.geoms[g].rbound) return false;
    return true;
}

// An update's host half: the tables of (trial, world) by the builder that made `cur`, checked to
// have cur's shape.  The caller adopts trial, world and out; a failure (message set) leaves all as
// they were.
inline int chain_update(const ChainTables& cur, const sspp_model& trial, const std::vector<double>& world, ChainTables& out) {
    if (int rc = chain_build(trial, cur.D, out, world.data())) return rc;
    if (!chain_same_shape(cur, out)) return sspp::set_error(SSPP_E_INVAL, "sspp_chain: a world changed the shape of the tables");
    return SSPP_OK;
}

}  // namespace sspc
