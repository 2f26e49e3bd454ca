// Host-only run of the contact report (tests/test_contact_report_host.py): the factored scene builder
// (sspp_scene_build.h) and the report's per-pose routine (sspr::pose_report, sspp_report.h) — the
// code the report kernels loop over — on the CPU, without a GPU.
//
//   check_report input.txt
// input.txt, whitespace-separated (the test writes it; doubles with 17 significant digits):
//   mode arg                     0: arg = dof; 1: arg = the moving body's id
//   nbody  then per body:  parent jnt_type qpos_adr  pos[3] quat[4]
//   ngeom  then per geom:  type body contype conaffinity  size[3] pos[3] quat[4] margin
//   nexclude then the body id pairs;  nq then qpos0
//   N D    then N poses of D values
// Prints
//   form F                       the collider form chosen for the scene (sspr::form_of)
//   pair g1 g2 moving1 moving2 margin            one per moving pair, report column order
//   static contacts cost                         the scene's env-env sums
//   spair g1 g2 margin contact deep              one per env-env pair
//   row HEX HEX                  per pose: the P contact counts and the P deep counts, two hex
//                                digits each ("-" for an empty table)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "sspp_scene_build.h"
#include "sspp_report.h"

namespace {
std::string g_err;
}
int sspp::set_error(int code, const std::string& msg) { g_err = msg; return code; }
void sspp::clear_error() { g_err.clear(); }

static std::string hex(const std::vector<uint8_t>& v) {
    if (v.empty()) return "-";
    std::string s;
    char b[3];
    for (uint8_t x : v) {
        std::snprintf(b, sizeof b, "%02x", x);
        s += b;
    }
    return s;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 3;
    auto I = [&]() { long long v = 0; in >> v; return (int)v; };
    auto F = [&]() { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); };
    const int mode = I(), arg = I();
    sspp_model m;
    const int nb = I();
    for (int b = 0; b < nb; ++b) {
        m.body_names.push_back("");
        m.body_parent.push_back(I());
        m.body_jnt_type.push_back(I());
        m.body_qpos_adr.push_back(I());
        for (int k = 0; k < 3; ++k) m.body_pos.push_back(F());
        for (int k = 0; k < 4; ++k) m.body_quat.push_back(F());
    }
    const int ng = I();
    for (int g = 0; g < ng; ++g) {
        m.geom_names.push_back("");
        m.geom_type.push_back(I());
        m.geom_body.push_back(I());
        m.geom_contype.push_back(I());
        m.geom_conaffinity.push_back(I());
        for (int k = 0; k < 3; ++k) m.geom_size.push_back(F());
        for (int k = 0; k < 3; ++k) m.geom_pos.push_back(F());
        for (int k = 0; k < 4; ++k) m.geom_quat.push_back(F());
        m.geom_margin.push_back(F());
    }
    const int ne = I();
    for (int e = 0; e < 2 * ne; ++e) m.exclude.push_back(I());
    const int nq = I();
    for (int k = 0; k < nq; ++k) m.qpos0.push_back(F());
    const int N = I(), D = I();
    std::vector<double> q((size_t)N * D);
    for (double& v : q) v = F();
    if (!in) return 4;

    std::vector<int> movers;
    if (mode == SSPP_MODE_QPOS) {
        for (int b = 1; b < nb; ++b)
            if (m.body_jnt_type[b] == 0 && m.body_qpos_adr[b] < arg) movers.push_back(b);
    } else {
        movers.push_back(arg);
    }
    if (movers.empty() || movers.size() > 2 || D != (mode == SSPP_MODE_QPOS ? arg : 4)) return 5;
    sspb::SceneTables t;
    if (sspb::scene_build(m, mode, movers, t)) {
        std::fprintf(stderr, "scene_build: %s\n", g_err.c_str());
        return 6;
    }
    // the scene as the library holds it, for the form its kernels take (sspk::kscene)
    sspp_scene sc;
    sc.mode = mode; sc.arg = arg; sc.dof = D; sc.count_static = 1;
    sc.geoms = t.geoms; sc.pairs = t.pairs; sc.movers = t.movers;
    sc.static_contacts = t.static_contacts; sc.static_cost = t.static_cost;
    const int form = sspr::form_of(sspk::kscene(&sc, mode == SSPP_MODE_BODY));
    std::printf("form %d\n", form);
    for (const sspd::DPair& pr : t.pairs) {
        const int go = t.geoms[pr.gm].orig;
        const bool gfirst = go < pr.oorig;
        std::printf("pair %d %d %d %d %.17g\n", gfirst ? go : pr.oorig, gfirst ? pr.oorig : go,
                    gfirst ? 1 : (int)(pr.omover >= 0), gfirst ? (int)(pr.omover >= 0) : 1, pr.margin);
    }
    std::printf("static %d %.17g\n", t.static_contacts, t.static_cost);
    for (const sspb::StaticPair& p : t.statics)
        std::printf("spair %d %d %.17g %d %d\n", p.g1, p.g2, p.margin, (int)p.contact, (int)p.deep);
    const int P = (int)t.pairs.size();
    std::vector<uint8_t> c(P), d(P);
    for (int i = 0; i < N; ++i) {
        sspr::dispatch_form(mode, (int)movers.size(), form, [&](auto nm, auto md, auto fm) {
            constexpr int NM = decltype(nm)::value, MODE = decltype(md)::value, FORM = decltype(fm)::value;
            double qv[sspr::kPoseVals<NM, MODE>];
            sspr::gather_pose<NM, MODE>(&q[(size_t)i * D], D, qv);
            sspr::pose_report<NM, MODE, FORM>(qv, D, t.geoms.data(), t.pairs.data(), t.movers.data(), P, c.data(),
                                              d.data());
        });
        std::printf("row %s %s\n", hex(c).c_str(), hex(d).c_str());
    }
    return 0;
}
