// sspp_chain_report.h — the contact report for arms: its per-pose routines (DESIGN.md §5 "Contact
// report for arms").
//
// chain_contact (sspp_chain.h) answers one bit per pose; these two answer per pair.  They run the
// test chain_contact runs — geom_pose, the bounding-sphere cull (a zero rbound is never culled),
// sspr::collide_form<false, kGeneric> with geom a first — but for every pair of the table:
//   chain_pair_report  contact[k] = collide_form<false>'s count, deep[k] = collide_form<true>'s *nd
//                      (contacts below -1e-3), for every k in [0, np), zeros included; nothing is
//                      skipped after a hit; a culled pair reports 0 / 0
//   chain_first_pair   the lowest k in contact, or -1
// Both are __host__ __device__ and templated on the table pointer types and the frame accessor, as
// chain_contact is: the kernels of sspp_chain_report.hip are thin loops around them, and
// tests/chain_report/check_chain_report.cpp runs the same code on the CPU.  The static-static pairs
// are not columns of the report: chain_build lists them with their counts (ChainTables::statics).
#pragma once
#include "sspp_chain.h"

namespace sspc {

// One pose (the frames fr) against pairs [0, np): contact[k] and, when deep is non-null, deep[k].
// The pair loop is wave-uniform in a kernel (records are scalar loads, the type branch is uniform);
// a geom's pose is kept while consecutive pairs share it.
template <class GP, class PP, class FR>
SSPP_HD void chain_pair_report(GP geoms, PP pairs, int np, const FR& fr, uint8_t* contact, uint8_t* deep) {
    int cur1 = -1, cur2 = -1;
    double p1[3], m1[9], p2[3], m2[9];
    for (int k = 0; k < np; ++k) {
        const int a = pairs[k].a, b = pairs[k].b;
        const double margin = pairs[k].margin;
        if (a != cur1) { geom_pose(geoms + a, fr, p1, m1); cur1 = a; }
        if (b != cur2) { geom_pose(geoms + b, fr, p2, m2); cur2 = b; }
        int nc = 0, nd = 0;
        bool near = true;
        const double r1 = geoms[a].rbound, r2 = geoms[b].rbound;
        if (r1 > 0.0 && r2 > 0.0) {
            const double dc[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
            const double thr = r1 + r2 + margin;
            near = !(dot3(dc, dc) > thr * thr);
        }
        if (near) {
            double s1[3], s2[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { s1[i] = geoms[a].size[i]; s2[i] = geoms[b].size[i]; }
            int unused = 0;
            nc = sspr::collide_form<false, sspr::kGeneric>(geoms[a].type, p1, m1, s1, geoms[b].type, p2, m2, s2, margin,
                                                           &unused);
            if (deep)
                sspr::collide_form<true, sspr::kGeneric>(geoms[a].type, p1, m1, s1, geoms[b].type, p2, m2, s2, margin, &nd);
        }
        contact[k] = (uint8_t)nc;
        if (deep) deep[k] = (uint8_t)nd;
    }
}

// The lowest column of [0, np) in contact at the frames fr, or -1: chain_contact's loop, keeping
// which pair it was.  A lane that has its pair skips the colliders of the later ones.
template <class GP, class PP, class FR>
SSPP_HD int chain_first_pair(GP geoms, PP pairs, int np, const FR& fr) {
    int cur1 = -1, cur2 = -1, first = -1;
    double p1[3], m1[9], p2[3], m2[9];
    for (int k = 0; k < np; ++k) {
        const int a = pairs[k].a, b = pairs[k].b;
        const double margin = pairs[k].margin;
        if (a != cur1) { geom_pose(geoms + a, fr, p1, m1); cur1 = a; }
        if (b != cur2) { geom_pose(geoms + b, fr, p2, m2); cur2 = b; }
        if (first >= 0) continue;
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
        if (nc > 0) first = k;
    }
    return first;
}

}  // namespace sspc
