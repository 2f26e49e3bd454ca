// Host build of the device narrowphase for cylinder-cylinder pairs (tests/test_cylcyl_ref.py):
// reads cases "margin p1[3] m1[9] s1[3] p2[3] m2[9] s2[3]" (31 numbers, hex floats) from the file
// argv[1] and prints, per case, sspd::collide<false>'s contact count, collide<true>'s deep count,
// the stage of cyl_cyl_overlap that decided each (-1: the vertical closed form), and the
// decisions of the three axes a_1, a_2, a_1 x a_2 alone.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "sspp_device.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char tok[64];
    double v[31];
    long n = 0;
    for (;;) {
        int k = 0;
        for (; k < 31; ++k) {
            if (std::fscanf(f, "%63s", tok) != 1) break;
            v[k] = std::strtod(tok, nullptr);
        }
        if (k == 0) break;
        if (k != 31) return 3;
        const double margin = v[0];
        const double *p1 = v + 1, *m1 = v + 4, *s1 = v + 13, *p2 = v + 16, *m2 = v + 19, *s2 = v + 28;
        int nd0 = 0, nd1 = 0, st_c = -1, st_d = -1;
        const int nc = sspd::collide<false>(5, p1, m1, s1, 5, p2, m2, s2, margin, &nd0);
        sspd::collide<true>(5, p1, m1, s1, 5, p2, m2, s2, margin, &nd1);
        if (!(sspd::cyl_vertical(m1) && sspd::cyl_vertical(m2))) {
            sspd::cyl_cyl_overlap<false>(p1, m1, s1, p2, m2, s2, margin, &st_c);
            sspd::cyl_cyl_overlap<false>(p1, m1, s1, p2, m2, s2, sspd::kDeep, &st_d);
        }
        const sspd::CylCyl c = sspd::make_cylcyl(p1, m1, s1, p2, m2, s2);
        std::printf("%d %d %d %d %d %d\n", nc, nd1, st_c, st_d, sspd::cc_base_sep(c, margin) ? 0 : 1,
                    sspd::cc_base_sep(c, sspd::kDeep) ? 0 : 1);
        ++n;
    }
    std::fclose(f);
    std::fprintf(stderr, "cases %ld\n", n);
    return 0;
}
