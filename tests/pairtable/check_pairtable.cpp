// Host-only check of a job's pair tables (tests/test_pairtable_host.py): builds sspp_scene records
// by hand and prints, per table, what sspk's table_set derives — "np cb og feps" — then the index
// of the table launch_table picks for each kind of launch, then what kscene_job / scene_t_job hand
// a launch for a table with and without a device copy.  The expected values are worked out by hand
// in the test.
#include <cstdio>

#include "sspp_kern.h"

// the owning types report HIP failures through these (sspp_capi.cpp in the library)
int sspp::set_error(int code, const std::string&) { return code; }
void sspp::clear_error() {}

static sspd::DGeom geom(int type, double rbound) {
    sspd::DGeom g{};
    g.mat[0] = g.mat[4] = g.mat[8] = 1.0;
    g.type = type; g.mover = 0; g.rbound = rbound;  // pos = 0: no offset from the mover's root
    return g;
}
static sspd::DPair pair(int gm, int otype, double orbound, double margin) {
    sspd::DPair p{};
    p.gm = gm; p.go = 3; p.otype = otype; p.omover = -1;
    p.omat[0] = p.omat[4] = p.omat[8] = 1.0;
    p.orbound = orbound; p.margin = margin;
    return p;
}
// a host address (or none) as a stand-in for a buffer's device copy, counted as the buffer counts
// its own allocations, so that the release() below leaves the live count where it was
template <class T>
static void adopt(sspo::Dev<T>& d, T* p) {
    (void)d.release();
    d.p = p;
    if (p) sspo::live_add(sspo::kLiveDev, 1);
}
static void row(const sspp_scene* sc, std::vector<sspd::DPair> pairs) {
    PairTable t;
    t.np = 99; t.cb = 99; t.og = 99; t.feps = 99.0;  // table_set must overwrite every one
    table_set(t, sc, std::move(pairs));
    std::printf("%d %d %d %.17g\n", t.np, t.cb, t.og, t.feps);
}

int main() {
    // moving geoms: 0 a box (type 6), 1 a cylinder (5), 2 a capsule (3), 3 a box without a bounding radius
    sspp_scene s{};
    s.geoms = {geom(6, 0.5), geom(5, 0.25), geom(3, 0.125), geom(6, 0.0)};
    const sspd::DPair box_cyl = pair(0, 5, 0.5, 0.0), cyl_cyl = pair(1, 5, 1.0, 0.25), cap_box = pair(2, 6, 0.25, 0.0),
                      box_box = pair(0, 6, 2.0, 0.5), small = pair(1, 6, 0.25, 0.0), cyl_box = pair(1, 6, 1.5, 0.25);
    row(&s, {box_cyl, cyl_cyl, cap_box, box_box});  // mixed
    row(&s, {box_box, box_box});                    // one geom
    row(&s, {box_cyl, cyl_box});                    // two geoms
    row(&s, {small});                               // extent below 1 m
    row(&s, {});                                    // empty
    row(nullptr, {});                               // empty, no scene
    row(&s, std::vector<sspd::DPair>(65, box_box)); // past 64 pairs
    row(&s, {box_box, pair(0, 6, 7.75, 0.0)});      // extent 8.25 m
    row(&s, {box_box, pair(3, 6, 1.0, 0.0)});       // a geom with rbound 0

    sspp_job j;
    for (int ctrl_in = 0; ctrl_in < 2; ++ctrl_in)
        for (int queries = 0; queries < 2; ++queries)
            std::printf("%d%s", (int)(&launch_table(&j, ctrl_in != 0, queries != 0) - j.tab), ctrl_in && queries ? "\n" : " ");

    // the scene's own pairs are {box_cyl, cyl_cyl}; a table with a device copy overrides them
    s.pairs = {box_cyl, cyl_cyl};
    adopt(s.d_pairs, &s.pairs[0]);  // (never read: only the pointers are compared; released below)
    j.scene = &s;
    PairTable& t = j.tab[kPairsSampled];
    table_set(t, &s, {box_box});
    for (int with_copy = 0; with_copy < 2; ++with_copy) {
        adopt(t.d, with_copy ? &t.h[0] : nullptr);
        const sspk::KScene k = sspk::kscene_job(&j, t);
        const sspk::SceneT T = sspk::scene_t_job(&j, t);
        std::printf("%d %d %d %d\n", k.npairs, k.cylbox, k.onegeom, T.pairs == t.d.p ? 1 : T.pairs == s.d_pairs.p ? 0 : -1);
    }
    // the host addresses stood in for device copies: their owners must not free them
    (void)t.d.release();
    (void)s.d_pairs.release();
    return sspo::g_live[sspo::kLiveDev].load() == 0 ? 0 : 1;
}
