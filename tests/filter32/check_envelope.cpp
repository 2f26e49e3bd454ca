// The FP32 filter against the FP64 narrowphase over the envelope f32_eps certifies (sspp_kern.h,
// DESIGN.md §5), where check_filter.cpp covers one corner of it.  Each configuration comes from a
// named stratum:
//   far     root target coordinates up to +-7.99 m, static partners up to +-16 m (a long box reached
//           from its end or its side), extents S <= 8
//   large   half extents of metres on either box, S spread over (1, 8]
//   offset  the moving box a geom up to 2 m off its mover's root with a generic local rotation
//   movers  the partner a geom of a second mover, composed from that mover's pose
//   plane   tilted planes (the ramp of the GPU scenes among them) whose origin lies up to 16 m per
//           axis from where the box touches them
// A configuration is built as scan_pairs32 / scan_pairs build it: both movers' poses through the
// kernel's 4-term spline (doubles for FP64, their float copies for FP32), the moving geom's pose
// as geom_pose (FP64) and SSPF_LOAD_GEOM / SSPF_GEOM_ROT (FP32: matvec3f of its offset, matmul3f of
// its rotation), a mover partner as the omover >= 0 branches do, root positions past kF32PosLimit
// left to FP64.  eps is the library's own: f32_eps of a one-pair table.  The touching distance is
// bisected on the FP64 decision (pair_near + narrowphase) and the pose placed +-10^U(-8,-1) max(1,S)
// from it; every certain FP32 decision must equal FP64's in both argument orders.  Per stratum one
// line: the counts, the mismatches and the largest |FP32 - FP64| decision quantity (SAT
// separations; corner heights for planes) per metre of max(1, S).  Built and run by
// tests/test_filter32.py.
#define SSPF_HOST_RSQ_JITTER
#include "sspp_kern.h"

#include <cstring>

#include "filter_common.h"

// the owning types report HIP failures through these (sspp_capi.cpp in the library)
int sspp::set_error(int code, const std::string&) { return code; }
void sspp::clear_error() {}

enum { kFar, kLarge, kOffset, kMovers, kPlane, kStrata };
static const char* const kNames[kStrata] = {"far", "large", "offset", "movers", "plane"};

struct Cfg {
    double ea[3], eb[3], margin;
    double gpos[3], gmat[9];   // the moving geom in its mover's frame
    bool relrot;
    bool plane, mover2;
    double pb[3], mb[9];       // the partner: world pose (static) or relative to the second mover
    double qbase[4], q2base[4], p2[3];
    double qsig, psig;
    double N[4], dq[2][4][4], dp[2][4][3];
};

struct Eval {
    double gp[3], gm[9], op[3], om[9];
    float gp32[3], gm32[9], op32[3], om32[9], root32[3];
    bool ok32;
};

// one mover's pose through the spline: the quaternion rows around qbase, the position rows so
// that the FP64 evaluation lands on `target` (up to rounding)
struct Pose {
    double p[3], m[9];
    float p32[3], m32[9];
    bool ok32;
};
static void quat_rows(const Cfg& c, int mv, double ctrl[4][7]) {
    const double* qb = mv ? c.q2base : c.qbase;
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) ctrl[r][3 + k] = qb[k] + c.dq[mv][r][k];
}
static Pose mover_pose(const Cfg& c, int mv, double ctrl[4][7], const double* target) {
    double shift[3] = {0, 0, 0};
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 3; ++k) shift[k] += c.N[r] * c.dp[mv][r][k];
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 3; ++k) ctrl[r][k] = target[k] + c.dp[mv][r][k] - shift[k];
    double qd[7];
    float q32[7];
    spline4(c.N, ctrl, 7, qd, q32);
    Pose e;
    double qq[4] = {qd[3], qd[4], qd[5], qd[6]};
    sspd::normalize4(qq);
    sspd::quat2mat(qq, e.m);
    e.ok32 = sspf::quat_rot32(q32 + 3, e.m32);
    for (int k = 0; k < 3; ++k) {
        e.p[k] = qd[k];
        e.p32[k] = q32[k];
        e.ok32 = e.ok32 && std::fabs(q32[k]) <= kF32PosLimit;  // mover_poses32
    }
    return e;
}

// the pair with the moving geom's centre at gtarget (its root at gtarget - R gpos)
static Eval make_eval(const Cfg& c, const double* gtarget) {
    double ctrl[4][7];
    quat_rows(c, 0, ctrl);
    // the rotation does not depend on the position rows: evaluate it first for the root's target
    double zero[3] = {0, 0, 0}, t[3], root[3];
    const Pose r0 = mover_pose(c, 0, ctrl, zero);
    sspd::matvec3(r0.m, c.gpos, t);
    for (int k = 0; k < 3; ++k) root[k] = gtarget[k] - t[k];
    const Pose a = mover_pose(c, 0, ctrl, root);
    Eval e;
    e.ok32 = a.ok32;
    for (int k = 0; k < 3; ++k) e.root32[k] = a.p32[k];
    // geom_pose / SSPF_LOAD_GEOM, SSPF_GEOM_ROT
    float fpos[3], fmat[9], t32[3];
    for (int k = 0; k < 3; ++k) fpos[k] = (float)c.gpos[k];
    for (int k = 0; k < 9; ++k) fmat[k] = (float)c.gmat[k];
    sspd::matvec3(a.m, c.gpos, t);
    sspf::matvec3f(a.m32, fpos, t32);
    for (int k = 0; k < 3; ++k) { e.gp[k] = a.p[k] + t[k]; e.gp32[k] = a.p32[k] + t32[k]; }
    if (c.relrot) {
        sspd::matmul3(a.m, c.gmat, e.gm);
        sspf::matmul3f(a.m32, fmat, e.gm32);
    } else {
        for (int k = 0; k < 9; ++k) { e.gm[k] = a.m[k]; e.gm32[k] = a.m32[k]; }
    }
    float fopos[3], fomat[9];
    for (int k = 0; k < 3; ++k) fopos[k] = (float)c.pb[k];
    for (int k = 0; k < 9; ++k) fomat[k] = (float)c.mb[k];
    if (c.mover2) {
        quat_rows(c, 1, ctrl);
        const Pose b = mover_pose(c, 1, ctrl, c.p2);
        e.ok32 = e.ok32 && b.ok32;
        sspd::matvec3(b.m, c.pb, t);
        sspf::matvec3f(b.m32, fopos, t32);
        for (int k = 0; k < 3; ++k) { e.op[k] = b.p[k] + t[k]; e.op32[k] = b.p32[k] + t32[k]; }
        sspd::matmul3(b.m, c.mb, e.om);
        sspf::matmul3f(b.m32, fomat, e.om32);
    } else {
        for (int k = 0; k < 3; ++k) { e.op[k] = c.pb[k]; e.op32[k] = fopos[k]; }
        for (int k = 0; k < 9; ++k) { e.om[k] = c.mb[k]; e.om32[k] = fomat[k]; }
    }
    return e;
}

// the 8 corner heights col_plane_box / plane_box32 compare with the margin
template <class T>
static void corner_heights(const T* pp, const T* pm, const T* bp, const T* bm, const T* e, T* out) {
    const T n[3] = {pm[2], pm[5], pm[8]};
    const T d0 = (bp[0] - pp[0]) * n[0] + (bp[1] - pp[1]) * n[1] + (bp[2] - pp[2]) * n[2];
    T a[3];
    for (int j = 0; j < 3; ++j) a[j] = (n[0] * bm[j] + n[1] * bm[3 + j] + n[2] * bm[6 + j]) * e[j];
    for (int k = 0; k < 8; ++k)
        out[k] = d0 + ((k & 1) ? a[0] : -a[0]) + ((k & 2) ? a[1] : -a[1]) + ((k & 4) ? a[2] : -a[2]);
}

static double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
static void unit_dir(double* d) {
    double n;
    do {
        for (int k = 0; k < 3; ++k) d[k] = U(-1, 1);
        n = norm3(d);
    } while (n < 0.1 || n > 1.0);
    for (int k = 0; k < 3; ++k) d[k] /= n;
}
static void ident(double* m) { for (int k = 0; k < 9; ++k) m[k] = (k % 4 == 0) ? 1.0 : 0.0; }
// a coordinate of the certified cube, half of them in its outer shell
static double cube_coord(double lim) {
    const double v = U01(g_rng) < 0.5 ? U(lim - 0.5, lim) : U(0.0, lim);
    return U01(g_rng) < 0.5 ? -v : v;
}

struct Stat { long tot = 0, hit = 0, no = 0, amb = 0, outside = 0, notok = 0, bad = 0; double err = 0.0, smax = 0.0, root = 0.0, partner = 0.0; };

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 30000;
    const double margins[] = {0.0, 0.0, 0.001, 0.1};
    const double qsigs[] = {0.0, 1e-7, 1e-4, 0.02, 0.08, 0.5};
    const double ramp[4] = {0.9950, 0.0998, 0.0, 0.0};  // the tilted plane of the GPU scenes
    sspp_scene sc{};
    sc.geoms.resize(1);
    long total_bad = 0;
    for (int st = 0; st < kStrata; ++st) {
        if (argc > 2 && std::strcmp(argv[2], kNames[st]) != 0) continue;
        g_rng.seed(20261020 + st);
        Stat s;
        for (long it = 0; it < n; ++it) {
            Cfg c{};
            c.plane = st == kPlane;
            c.mover2 = st == kMovers;
            c.margin = margins[it % 4];
            c.qsig = qsigs[(it / 4) % 6];
            c.psig = U01(g_rng) < 0.5 ? 0.0 : 0.05;
            ident(c.gmat);
            for (int k = 0; k < 3; ++k) { c.ea[k] = U(0.005, 0.3); c.eb[k] = U(0.005, 0.6); }
            // the partner's rotation: identity, a yaw, or generic
            const int orient = (int)(U01(g_rng) * 3);
            double qb[4] = {1, 0, 0, 0};
            if (orient == 1) { const double h = U(-M_PI, M_PI) / 2; qb[0] = std::cos(h); qb[3] = std::sin(h); }
            else if (orient == 2) rand_quat(qb);
            double dir[3];
            unit_dir(dir);
            double contact[3];  // about where the two touch
            for (int k = 0; k < 3; ++k) contact[k] = U(-1.0, 1.0);
            if (st == kFar) {
                for (int k = 0; k < 3; ++k) contact[k] = cube_coord(7.99);
                c.eb[0] = U(0.5, 7.3);
                c.eb[1] = U(0.05, 1.0);
                c.eb[2] = U(0.05, 1.0);
            } else if (st == kLarge) {
                // S = ra + rb + margin over (1, 8]: the two radii share a drawn S
                const double S = U(1.0, 7.9), fa = U(0.1, 0.9);
                double sa[3], sb[3];
                for (int k = 0; k < 3; ++k) { sa[k] = U(0.05, 1.0); sb[k] = U(0.05, 1.0); }
                for (int k = 0; k < 3; ++k) {
                    c.ea[k] = sa[k] / norm3(sa) * fa * (S - c.margin);
                    c.eb[k] = sb[k] / norm3(sb) * (1.0 - fa) * (S - c.margin);
                }
                for (int k = 0; k < 3; ++k) contact[k] = U(-4.0, 4.0);
            } else if (st == kOffset || st == kMovers) {
                if (st == kOffset || U01(g_rng) < 0.5) {
                    double o[3], q[4];
                    unit_dir(o);
                    const double len = U(0.1, 2.0);
                    for (int k = 0; k < 3; ++k) c.gpos[k] = o[k] * len;
                    rand_quat(q);
                    sspd::quat2mat(q, c.gmat);
                    c.relrot = true;
                }
                for (int k = 0; k < 3; ++k) contact[k] = U(-3.0, 3.0);
            } else if (st == kPlane) {
                for (int k = 0; k < 3; ++k) contact[k] = cube_coord(7.5);
                const int tilt = (int)(U01(g_rng) * 4);
                if (tilt == 0) for (int k = 0; k < 4; ++k) qb[k] = ramp[k];
                else if (tilt == 1) { const double h = U(-0.6, 0.6) / 2; qb[0] = std::cos(h); qb[1] = std::sin(h); qb[2] = qb[3] = 0; }
                else rand_quat(qb);
                double s2 = 0;
                for (int k = 0; k < 4; ++k) s2 += qb[k] * qb[k];
                for (int k = 0; k < 4; ++k) qb[k] /= std::sqrt(s2);
                if (U01(g_rng) < 0.3) {   // sometimes larger boxes on the plane
                    const double f = U(1.0, 10.0);
                    for (int k = 0; k < 3; ++k) c.ea[k] *= f;
                }
            }
            sspd::quat2mat(qb, c.mb);
            // the moving box's orientation: aligned with the partner's, or random, then perturbed
            if (U01(g_rng) < 0.5) for (int k = 0; k < 4; ++k) c.qbase[k] = qb[k];
            else rand_quat(c.qbase);
            rand_quat(c.q2base);
            c.N[0] = 1; c.N[1] = c.N[2] = c.N[3] = 0;
            if (U01(g_rng) < 0.8) {
                double sum = 0;
                for (int r = 0; r < 4; ++r) { c.N[r] = U(0, 1); sum += c.N[r]; }
                for (int r = 0; r < 4; ++r) c.N[r] /= sum;
            }
            for (int mv = 0; mv < 2; ++mv)
                for (int r = 0; r < 4; ++r) {
                    for (int k = 0; k < 4; ++k) c.dq[mv][r][k] = c.qsig * U(-1, 1);
                    for (int k = 0; k < 3; ++k) c.dp[mv][r][k] = c.psig * U(-1, 1);
                }
            if (st == kFar && U01(g_rng) < 0.6) {
                // along the long box's axis (its end reached from up to 7.8 m away) or across it
                const double l[3] = {U01(g_rng) < 0.5 ? 1.0 : U(-0.2, 0.2), U(-0.3, 0.3), U(-0.3, 0.3)};
                const double sg = U01(g_rng) < 0.5 ? -1.0 : 1.0;
                for (int k = 0; k < 3; ++k) dir[k] = sg * (c.mb[3 * k] * l[0] + c.mb[3 * k + 1] * l[1] + c.mb[3 * k + 2] * l[2]);
                const double dn = norm3(dir);
                for (int k = 0; k < 3; ++k) dir[k] /= dn;
            }
            const double ra = norm3(c.ea), rb = c.plane ? 0.0 : norm3(c.eb);
            double nrm[3] = {c.mb[2], c.mb[5], c.mb[8]}, climb = 1.0;
            if (c.plane) {
                climb = dir[0] * nrm[0] + dir[1] * nrm[1] + dir[2] * nrm[2];
                while (std::fabs(climb) < 0.2) {
                    unit_dir(dir);
                    climb = dir[0] * nrm[0] + dir[1] * nrm[1] + dir[2] * nrm[2];
                }
                if (climb < 0) { for (int k = 0; k < 3; ++k) dir[k] = -dir[k]; climb = -climb; }
                // the origin: `contact` moved within the plane, up to 16 m per axis and within the
                // 16 m of the origin that f32_eps asks of a partner
                for (int tries = 0;; ++tries) {
                    const double a = U(-16, 16) * (tries > 4 ? 0.1 : 1.0), b = U(-16, 16) * (tries > 4 ? 0.1 : 1.0);
                    bool ok = true;
                    for (int k = 0; k < 3; ++k) {
                        const double d = a * c.mb[3 * k] + b * c.mb[3 * k + 1];
                        c.pb[k] = contact[k] + d;
                        ok = ok && std::fabs(d) <= 16.0 && std::fabs(c.pb[k]) <= 16.0;
                    }
                    if (ok) break;
                }
            } else if (c.mover2) {
                // the partner hangs up to 2 m off the second mover's root
                double o[3];
                unit_dir(o);
                const double len = U(0.0, 2.0);
                for (int k = 0; k < 3; ++k) { c.pb[k] = o[k] * len; c.p2[k] = contact[k]; }
            } else {
                for (int k = 0; k < 3; ++k) c.pb[k] = contact[k];
            }
            // the library's eps for this pair as a one-pair table
            sspd::DGeom& G = sc.geoms[0];
            G = sspd::DGeom{};
            sspd::DPair pr{};
            for (int k = 0; k < 3; ++k) { G.pos[k] = c.gpos[k]; G.size[k] = c.ea[k]; pr.osize[k] = c.eb[k]; }
            for (int k = 0; k < 9; ++k) { G.mat[k] = c.gmat[k]; pr.omat[k] = c.mb[k]; }
            G.type = 6; G.mover = 0; G.relrot = c.relrot; G.rbound = ra; G.reach = norm3(c.gpos);
            pr.gm = 0; pr.otype = c.plane ? 0 : 6; pr.omover = c.mover2 ? 1 : -1;
            pr.margin = c.margin; pr.orbound = rb;
            Eval e;
            double lo = 0.0, hi = 0.0, base[3];
            auto contact64 = [&](const Eval& v, bool swap) -> bool {
                int nd = 0;
                if (!sspd::pair_near(pr, ra, v.gp, v.op, v.om)) return false;
                if (c.plane) return sspd::col_plane_box(v.op, v.om, v.gp, v.gm, c.ea, c.margin, &nd) > 0;
                return swap ? sspd::sat_box_box(v.op, v.om, c.eb, v.gp, v.gm, c.ea, c.margin)
                            : sspd::sat_box_box(v.gp, v.gm, c.ea, v.op, v.om, c.eb, c.margin);
            };
            auto at = [&](double t) {
                double g[3];
                for (int k = 0; k < 3; ++k) g[k] = base[k] + t * dir[k];
                return make_eval(c, g);
            };
            // touching distance along dir from the partner's centre (a point of the plane): FP64 bisection
            auto bisect = [&]() -> bool {
                lo = 0.0;
                hi = (ra + rb + c.margin + 1.0) / climb;
                if (!contact64(at(lo), false) || contact64(at(hi), false)) return false;
                for (int k = 0; k < 60; ++k) {
                    const double mid = 0.5 * (lo + hi);
                    if (contact64(at(mid), false)) lo = mid; else hi = mid;
                }
                return true;
            };
            if (c.mover2) {
                const Eval v = make_eval(c, contact);
                for (int k = 0; k < 3; ++k) base[k] = v.op[k];
            } else {
                for (int k = 0; k < 3; ++k) base[k] = contact[k];
            }
            if (st == kFar) {
                // the touching pose, not the partner, lies at `contact`: move the partner back by
                // the touching distance (translation-invariant up to rounding), then bisect where it is
                if (!bisect()) { ++s.outside; continue; }
                for (int k = 0; k < 3; ++k) c.pb[k] = base[k] = contact[k] - hi * dir[k];
            }
            for (int k = 0; k < 3; ++k) pr.opos[k] = c.pb[k];
            const double eps64 = f32_eps(&sc, {pr});
            if (eps64 <= 0.0 || !bisect()) { ++s.outside; continue; }
            const double S = eps64 / kF32EpsPerMetre;
            const double off = (U01(g_rng) < 0.5 ? -1 : 1) * std::pow(10.0, U(-8.0, -1.0)) * S;
            e = at(0.5 * (lo + hi) + off);
            if (!e.ok32) { ++s.notok; continue; }
            ++s.tot;
            s.smax = std::max(s.smax, S);
            for (int k = 0; k < 3; ++k) {
                s.root = std::max(s.root, (double)std::fabs(e.root32[k]));
                s.partner = std::max(s.partner, std::fabs(pr.opos[k]));
            }
            const float eps = (float)eps64;
            float ea32[3], eb32[3];
            for (int k = 0; k < 3; ++k) { ea32[k] = (float)c.ea[k]; eb32[k] = (float)c.eb[k]; }
            // the kernel's FP32 decision (scan_pairs32): the certified culls, then the narrowphase
            const int nr = sspf::pair_near32((float)rb, pr.otype, (float)c.margin, eb32, (float)ra, e.gp32, e.op32, e.om32,
                                             eps, (float)sspd::kHullPad);
            int r32 = sspf::kNo;
            if (nr != sspf::kNo) {
                if (c.plane) r32 = sspf::collide32(0, e.op32, e.om32, eb32, 6, e.gp32, e.gm32, ea32, (float)c.margin, eps);
                else r32 = sspf::collide32(6, e.gp32, e.gm32, ea32, 6, e.op32, e.om32, eb32, (float)c.margin, eps);
                if (r32 == sspf::kHit && nr == sspf::kAmb) r32 = sspf::kAmb;
            }
            const bool c64a = contact64(e, false), c64b = c.plane ? c64a : contact64(e, true);
            if (c.plane) {
                double h64[8];
                float h32[8];
                corner_heights<double>(e.op, e.om, e.gp, e.gm, c.ea, h64);
                corner_heights<float>(e.op32, e.om32, e.gp32, e.gm32, ea32, h32);
                for (int a = 0; a < 8; ++a) s.err = std::max(s.err, std::fabs((double)h32[a] - h64[a]) / S);
            } else {
                double s64[15];
                float s32[15];
                bool u64[15], u32[15];
                sat_seps<double>(e.gp, e.gm, c.ea, e.op, e.om, c.eb, s64, u64);
                sat_seps<float>(e.gp32, e.gm32, ea32, e.op32, e.om32, eb32, s32, u32);
                for (int a = 0; a < 15; ++a)
                    if (u64[a] && u32[a]) s.err = std::max(s.err, std::fabs((double)s32[a] - s64[a]) / S);
            }
            if (r32 == sspf::kAmb) { ++s.amb; continue; }
            if (r32 == sspf::kHit) ++s.hit; else ++s.no;
            const bool want = r32 == sspf::kHit;
            if (c64a != want || c64b != want) {
                ++s.bad;
                if (s.bad <= 10)
                    printf("MISMATCH %s it %ld r32 %d fp64 %d/%d off %.3e S %.3f margin %g qsig %g\n", kNames[st], it, r32,
                           c64a, c64b, off, S, c.margin, c.qsig);
            }
        }
        printf("stratum %s tested %ld certain-hit %ld certain-no %ld ambiguous %ld outside %ld unfiltered-pose %ld "
               "largest-S %.3f largest-root %.3f largest-partner %.3f error-per-metre %.3e mismatches %ld\n",
               kNames[st], s.tot, s.hit, s.no, s.amb, s.outside, s.notok, s.smax, s.root, s.partner, s.err, s.bad);
        total_bad += s.bad;
    }
    return total_bad ? 1 : 0;
}
