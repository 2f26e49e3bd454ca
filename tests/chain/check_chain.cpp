// Host-only run of the articulated movers' code (tests/test_chain_host.py, tests/test_gpu_chain.py):
// the MJCF loader (mjcf.cpp, compiled beside this file), sspc::chain_build and the per-pose routines
// sspc::chain_fk / geom_pose / chain_contact (sspp_chain.h) — the code the chain kernels loop over —
// and, for the frozen twin, sspb::scene_build's env-env path.  No GPU.
//
//   check_chain load strict|joints model.xml
//       rc R / err MESSAGE, then (rc 0): nq, qpos0, one line per body (jnt_type qpos_adr) and per joint
//   check_chain chain model.xml D count_static poses.bin out
//       poses.bin: raw doubles [N][D].  Prints rc / err, info, one `pair g1 g2 moving1 moving2 margin`
//       per table row; writes out.fk (raw doubles [N][ngeom][3 + 9]) and out.hit (N bytes)
//   check_chain twin model.xml poses.bin out
//       a free-body model (strict loader); poses.bin: raw doubles [N][nq].  Per pose the model's qpos0
//       is replaced and scene_build run without movers: prints `spair g1 g2` per env-env pair, writes
//       out.contact (bytes [N][pairs], collide<false>'s counts)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "sspp_scene_build.h"
#include "sspp_chain.h"

namespace {
std::string g_err;

std::vector<double> read_doubles(const char* path) {
    std::ifstream in(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<double> v(raw.size() / sizeof(double));
    if (!v.empty()) std::memcpy(v.data(), raw.data(), v.size() * sizeof(double));
    return v;
}
template <class T>
bool write_raw(const std::string& path, const std::vector<T>& v) {
    std::ofstream out(path, std::ios::binary);
    if (!v.empty()) out.write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
    return (bool)out;
}
}  // namespace
int sspp::set_error(int code, const std::string& msg) { g_err = msg; return code; }
void sspp::clear_error() { g_err.clear(); }

static int report_rc(int rc) {
    std::printf("rc %d\n", rc);
    if (rc) std::printf("err %s\n", g_err.c_str());
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string mode = argv[1];
    if (mode == "load") {
        sspp_model m;
        if (report_rc(sspp::load_mjcf(argv[3], m, std::string(argv[2]) == "joints"))) return 0;
        std::printf("nq %d\n", (int)m.qpos0.size());
        std::printf("qpos0");
        for (double v : m.qpos0) std::printf(" %.17g", v);
        std::printf("\n");
        for (int b = 0; b < m.nbody(); ++b)
            std::printf("body %d %d %d %d %d\n", b, m.body_jnt_type[b], m.body_qpos_adr[b], m.body_jnt_adr[b],
                        m.body_jnt_num[b]);
        for (int j = 0; j < m.njnt(); ++j)
            std::printf("jnt %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %s\n", m.jnt_type[j], m.jnt_body[j],
                        m.jnt_qpos_adr[j], m.jnt_axis[3 * j], m.jnt_axis[3 * j + 1], m.jnt_axis[3 * j + 2],
                        m.jnt_pos[3 * j], m.jnt_pos[3 * j + 1], m.jnt_pos[3 * j + 2], m.jnt_names[j].c_str());
        return 0;
    }
    if (mode == "chain") {
        if (argc < 7) return 2;
        sspp_model m;
        if (report_rc(sspp::load_mjcf(argv[2], m, true))) return 0;
        const int D = std::atoi(argv[3]), count_static = std::atoi(argv[4]);
        sspc::ChainTables t;
        if (report_rc(sspc::chain_build(m, D, t))) return 0;
        const int nd = (int)t.bodies.size(), ng = (int)t.geoms.size(), np = (int)t.pairs.size();
        std::printf("info %d %d %d %d %d %d %d\n", nd, ng, t.n_moving_geoms, t.n_static_geoms, np, t.n_static_pairs,
                    t.static_contacts);
        for (const sspc::CPair& p : t.pairs) {
            const int g1 = std::min(p.a, p.b), g2 = std::max(p.a, p.b);
            std::printf("pair %d %d %d %d %.17g\n", g1, g2, (int)(t.geoms[g1].slot >= 0), (int)(t.geoms[g2].slot >= 0),
                        p.margin);
        }
        const std::vector<double> q = read_doubles(argv[5]);
        const size_t N = q.size() / (size_t)D;
        const int static_block = (count_static && t.static_contacts > 0) ? 1 : 0;
        std::vector<double> fk(N * (size_t)ng * 12), frames((size_t)7 * std::max(1, nd));
        std::vector<uint8_t> hit(N);
        for (size_t i = 0; i < N; ++i) {
            const double* qi = &q[i * D];
            const sspc::ArrayFrames fr{frames.data()};
            sspc::chain_fk(t.bodies.data(), t.joints.data(), nd, D, [qi](int adr) { return qi[adr]; }, fr);
            for (int g = 0; g < ng; ++g) {
                double* o = &fk[(i * ng + g) * 12];
                sspc::geom_pose(t.geoms.data() + g, fr, o, o + 3);
            }
            hit[i] = (uint8_t)((sspc::chain_contact(t.geoms.data(), t.pairs.data(), np, fr) || static_block) ? 1 : 0);
        }
        const std::string out = argv[6];
        return write_raw(out + ".fk", fk) && write_raw(out + ".hit", hit) ? 0 : 7;
    }
    if (mode == "twin") {
        if (argc < 5) return 2;
        sspp_model m;
        if (report_rc(sspp::load_mjcf(argv[2], m, false))) return 0;
        const int nq = (int)m.qpos0.size();
        const std::vector<double> q = read_doubles(argv[3]);
        const size_t N = nq ? q.size() / (size_t)nq : 0;
        std::vector<uint8_t> contact;
        size_t P = 0;
        for (size_t i = 0; i < N; ++i) {
            m.qpos0.assign(q.begin() + i * nq, q.begin() + (i + 1) * nq);
            sspb::SceneTables t;
            if (const int rc = sspb::scene_build(m, SSPP_MODE_QPOS, std::vector<int>(), t)) {
                report_rc(rc);
                return 0;
            }
            if (i == 0) {
                P = t.statics.size();
                for (const sspb::StaticPair& p : t.statics) std::printf("spair %d %d\n", p.g1, p.g2);
                contact.assign(N * P, 0);
            }
            if (t.statics.size() != P) return 8;
            for (size_t k = 0; k < P; ++k) contact[i * P + k] = t.statics[k].contact;
        }
        return write_raw(std::string(argv[4]) + ".contact", contact) ? 0 : 7;
    }
    return 2;
}
