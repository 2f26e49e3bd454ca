// Host build of the device narrowphase on boundary poses (tests/test_boundary_poses.py): reads
// cases "t1 t2 margin p1[3] m1[9] s1[3] p2[3] m2[9] s2[3] mover" (34 numbers, hex floats; geom 1
// first by (type, model index), mover = 1 or 2: which of them moves) from the file argv[1] and
// prints, per case,
//   collide<false>'s contact count, collide<true>'s deep count,
//   the deep counts of collide<true, 2> (cylinder-box: cb_upright_sd only), collide<true, 1, true>
//   (the candidate search out of line) and collide<true, 1, false, false, true> (upright box-box),
//   each -1 where the variant's precondition does not hold for the case,
//   and pair_near's verdict for the pair as the kernels' tables hold it (mover, partner).
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "sspp_device.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char tok[64];
    double v[34];
    long n = 0;
    for (;;) {
        int k = 0;
        for (; k < 34; ++k) {
            if (std::fscanf(f, "%63s", tok) != 1) break;
            v[k] = std::strtod(tok, nullptr);
        }
        if (k == 0) break;
        if (k != 34) return 3;
        const int t1 = (int)v[0], t2 = (int)v[1], mover = (int)v[33];
        const double margin = v[2];
        const double *p1 = v + 3, *m1 = v + 6, *s1 = v + 15, *p2 = v + 18, *m2 = v + 21, *s2 = v + 30;
        if (!sspd::pair_supported(t1, t2) || t1 > t2 || (mover != 1 && mover != 2)) return 4;
        int nd0 = 0, nd = 0, nd_cb2 = -1, nd_out = 0, nd_up = -1;
        const int nc = sspd::collide<false>(t1, p1, m1, s1, t2, p2, m2, s2, margin, &nd0);
        sspd::collide<true>(t1, p1, m1, s1, t2, p2, m2, s2, margin, &nd);
        sspd::collide<true, 1, true>(t1, p1, m1, s1, t2, p2, m2, s2, margin, &nd_out);
        if (t1 != 5 || (sspd::cyl_vertical(m1) && sspd::upright3(m2)))
            sspd::collide<true, 2>(t1, p1, m1, s1, t2, p2, m2, s2, margin, &nd_cb2);
        if (t1 != 6 || (sspd::upright3(m1) && sspd::upright3(m2)))
            sspd::collide<true, 1, false, false, true>(t1, p1, m1, s1, t2, p2, m2, s2, margin, &nd_up);
        // the pair as a table row: the partner's data inlined, the mover's bounding radius beside it
        const int to = mover == 1 ? t2 : t1;
        const double *gp = mover == 1 ? p1 : p2, *gs = mover == 1 ? s1 : s2;
        const double *op = mover == 1 ? p2 : p1, *om = mover == 1 ? m2 : m1, *os = mover == 1 ? s2 : s1;
        sspd::DPair pr = {};
        pr.otype = to;
        pr.margin = margin;
        for (int i = 0; i < 3; ++i) { pr.opos[i] = op[i]; pr.osize[i] = os[i]; }
        for (int i = 0; i < 9; ++i) pr.omat[i] = om[i];
        pr.orbound = sspd::geom_rbound(to, os);
        const double rg = sspd::geom_rbound(mover == 1 ? t1 : t2, gs);
        const int near = sspd::pair_near(pr, rg, gp, op, om) ? 1 : 0;
        std::printf("%d %d %d %d %d %d\n", nc, nd, nd_cb2, nd_out, nd_up, near);
        ++n;
    }
    std::fclose(f);
    std::fprintf(stderr, "cases %ld\n", n);
    return 0;
}
