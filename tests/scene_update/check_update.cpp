// Host-only check of scene re-posing (tests/test_scene_update_host.py): the product's MJCF loader and
// the factored host table builder (sspp_scene_build.h), without a GPU.
//
//   check_update base.xml fresh.xml mode arg [op ...]
// mode 0: arg = dof (SamplingPathPlanner scene); mode 1: arg = a body's name (TaskSpacePlanner scene).
// Ops, applied in order to a copy of base.xml's model, as sspp_scene_set_qpos / _set_body_pose apply
// them to a scene's copy:
//   qpos v0 .. v{nq-1}                    model_set_qpos
//   body NAME px py pz qw qx qy qz       model_set_body_pose (NAME "#k": body id k, unchecked)
// Prints
//   rc <code> ...                         one per op
//   same <geoms> <pairs> <movers> <visit> <counts>   the re-posed tables against the tables built
//                                         fresh from fresh.xml, byte for byte (1 / 0 each)
//   base <geoms> <pairs> ...              the same against base.xml's own tables
//   static <contacts> <cost>              the re-posed scene's env-env contacts and cost
//   geom NAME x y z                       every geom's position in the re-posed tables
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sspp_scene_build.h"

namespace {
std::string g_err;
}
int sspp::set_error(int code, const std::string& msg) { g_err = msg; return code; }
void sspp::clear_error() { g_err.clear(); }

template <class T>
static int same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}
static void compare(const char* tag, const sspb::SceneTables& a, const sspb::SceneTables& b) {
    const int counts = a.n_moving_geoms == b.n_moving_geoms && a.n_static_geoms == b.n_static_geoms &&
                       a.n_static_pairs == b.n_static_pairs && a.static_contacts == b.static_contacts &&
                       std::memcmp(&a.static_cost, &b.static_cost, sizeof(double)) == 0;
    std::printf("%s %d %d %d %d %d\n", tag, same(a.geoms, b.geoms), same(a.pairs, b.pairs), same(a.movers, b.movers),
                same(a.visit, b.visit), counts);
}

static int movers_of(const sspp_model& m, int mode, const char* arg, std::vector<int>& out) {
    if (mode == SSPP_MODE_QPOS) {
        const int dof = std::atoi(arg);
        for (int b = 1; b < m.nbody(); ++b)
            if (m.body_jnt_type[b] == 0 && m.body_qpos_adr[b] < dof) out.push_back(b);
        return 0;
    }
    for (int b = 1; b < m.nbody(); ++b)
        if (m.body_names[b] == arg) { out.push_back(b); return 0; }
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    sspp_model base, fresh;
    if (sspp::load_mjcf(argv[1], base) != SSPP_OK || sspp::load_mjcf(argv[2], fresh) != SSPP_OK) {
        std::fprintf(stderr, "load: %s\n", g_err.c_str());
        return 3;
    }
    const int mode = std::atoi(argv[3]);
    std::vector<int> movers;
    if (movers_of(base, mode, argv[4], movers)) return 4;
    sspb::SceneTables t_base, t_fresh, t_re;
    if (sspb::scene_build(base, mode, movers, t_base) || sspb::scene_build(fresh, mode, movers, t_fresh)) return 5;
    sspp_model m = base;  // the scene's copy
    for (int i = 5; i < argc;) {
        int rc;
        if (!std::strcmp(argv[i], "qpos")) {
            std::vector<double> q;
            for (++i; i < argc && std::strcmp(argv[i], "qpos") && std::strcmp(argv[i], "body"); ++i) q.push_back(std::atof(argv[i]));
            rc = sspb::model_set_qpos(m, q.data(), (int)q.size());
        } else if (!std::strcmp(argv[i], "body") && i + 8 < argc) {
            int body = -1;
            if (argv[i + 1][0] == '#') body = std::atoi(argv[i + 1] + 1);
            else
                for (int b = 0; b < m.nbody(); ++b)
                    if (m.body_names[b] == argv[i + 1]) body = b;
            double v[7];
            for (int k = 0; k < 7; ++k) v[k] = std::atof(argv[i + 2 + k]);
            rc = sspb::model_set_body_pose(m, body, v, v + 3);
            i += 9;
        } else {
            return 6;
        }
        std::printf("rc %d %s\n", rc, g_err.c_str());
        g_err.clear();
    }
    if (sspb::scene_build(m, mode, movers, t_re)) return 7;
    compare("same", t_re, t_fresh);
    compare("base", t_re, t_base);
    std::printf("static %d %.17g\n", t_re.static_contacts, t_re.static_cost);
    for (const sspd::DGeom& g : t_re.geoms)
        std::printf("geom %s %.17g %.17g %.17g\n", m.geom_names[g.orig].c_str(), g.pos[0], g.pos[1], g.pos[2]);
    return 0;
}
