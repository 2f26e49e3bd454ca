// Host build of the device narrowphase for capsule pairs (tests/test_capsule_ref.py): reads
// cases "t1 t2 margin p1[3] m1[9] s1[3] p2[3] m2[9] s2[3]" (33 numbers, hex floats) from the
// file argv[1] and prints, per case, sspd::collide<false>'s contact count, collide<true>'s deep
// count, and the signed distance of every sphere test the rule ran (nan: not run).
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "sspp_device.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char tok[64];
    double v[33];
    long n = 0;
    for (;;) {
        int k = 0;
        for (; k < 33; ++k) {
            if (std::fscanf(f, "%63s", tok) != 1) break;
            v[k] = std::strtod(tok, nullptr);
        }
        if (k == 0) break;
        if (k != 33) return 3;
        const int t1 = (int)v[0], t2 = (int)v[1];
        const double margin = v[2];
        const double *p1 = v + 3, *m1 = v + 6, *s1 = v + 15, *p2 = v + 18, *m2 = v + 21, *s2 = v + 30;
        int nd0 = 0, nd1 = 0, ndx = 0;
        const int nc = sspd::collide<false>(t1, p1, m1, s1, t2, p2, m2, s2, margin, &nd0);
        sspd::collide<true>(t1, p1, m1, s1, t2, p2, m2, s2, margin, &nd1);
        double d[4] = {NAN, NAN, NAN, NAN};
        if (t1 == 0 && t2 == 3) sspd::col_plane_capsule(p1, m1, p2, m2, s2, margin, &ndx, d);
        else if (t1 == 2 && t2 == 3) sspd::col_sphere_capsule(p1, s1[0], p2, m2, s2, margin, &ndx, d);
        else if (t1 == 3 && t2 == 3) sspd::col_capsule_capsule(p1, m1, s1, p2, m2, s2, margin, &ndx, d);
        else if (t1 == 3 && t2 == 6) sspd::col_capsule_box(p1, m1, s1, p2, m2, s2, margin, &ndx, d);
        else return 4;
        std::printf("%d %d %.17g %.17g %.17g %.17g\n", nc, nd1, d[0], d[1], d[2], d[3]);
        ++n;
    }
    std::fclose(f);
    std::fprintf(stderr, "cases %ld\n", n);
    return 0;
}
