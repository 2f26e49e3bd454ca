// Host-only check of the TaskSpacePlanner kernel selection (tests/test_cylcyl_ref.py): builds
// sspp_scene records by hand — a mover cylinder (optionally rotated in its body) against a static
// cylinder and a static box, each vertical / upright or tilted — and prints, per scene,
// sspk::kscene's cylbox bits, cbup, upright and sspk::tsp_cbm (the CB the kernels are launched
// with), for the default and for the forced-generic selection.
#include <cstdio>

#include "sspp_kern.h"

static const double kI[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
// a rotation about x by 0.3 rad: m[5], m[7] non-zero (neither vertical nor upright)
static const double kTilt[9] = {1, 0, 0, 0, 0.955336489125606, -0.29552020666133955, 0, 0.29552020666133955, 0.955336489125606};
// a rotation about z: stays vertical / upright
static const double kYaw[9] = {0.8, -0.6, 0, 0.6, 0.8, 0, 0, 0, 1};

static sspd::DGeom geom(int type, const double* m, int relrot) {
    sspd::DGeom g{};
    for (int k = 0; k < 9; ++k) g.mat[k] = m[k];
    g.size[0] = 0.03; g.size[1] = 0.05; g.size[2] = 0.04;
    g.type = type; g.mover = 0; g.relrot = relrot;
    return g;
}
static sspd::DPair pair(int otype, const double* m) {
    sspd::DPair p{};
    p.gm = 0; p.go = 1; p.otype = otype; p.omover = -1;
    for (int k = 0; k < 9; ++k) p.omat[k] = m[k];
    return p;
}

int main() {
    // rows: mover geom rotation, static cylinder rotation (null: none), static box rotation (null: none)
    struct Row { const double* mg; int relrot; const double* cyl; const double* box; };
    const Row rows[] = {
        {kI, 0, kI, kYaw},       // vertical cylinders, upright box        -> 3
        {kI, 0, kYaw, nullptr},  // a yawed static cylinder is vertical    -> 3
        {kI, 0, kTilt, kYaw},    // tilted static cylinder                 -> 1
        {kTilt, 1, kI, nullptr}, // mover cylinder tilted in its body      -> 1
        {kI, 0, nullptr, kYaw},  // cylinder-box only, upright             -> 2
        {kI, 0, kI, kTilt},      // vertical cylinders, tilted box         -> 1
    };
    for (const Row& r : rows) {
        sspp_scene s{};
        s.geoms.push_back(geom(5, r.mg, r.relrot));
        if (r.cyl) s.pairs.push_back(pair(5, r.cyl));
        if (r.box) s.pairs.push_back(pair(6, r.box));
        for (int generic = 0; generic < 2; ++generic) {
            const sspk::KScene k = sspk::kscene(&s, true, generic != 0);
            std::printf("%d %d %d %d%s", k.cylbox, k.cbup, k.upright, sspk::tsp_cbm(k), generic ? "\n" : "  ");
        }
    }
    return 0;
}
