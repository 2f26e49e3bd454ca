// Host-only run of the contact report for arms (tests/test_chain_report_host.py,
// tests/test_gpu_chain_report.py): sspc::chain_build and the per-pose routines sspc::chain_fk /
// chain_pair_report / chain_first_pair (sspp_chain_report.h) — the code the report's kernels loop
// over — and, for the frozen twin, sspb::scene_build's env-env path with its per-pair counts.  No GPU.
//
//   check_chain_report chain model.xml D poses.bin out
//       poses.bin: raw doubles [N][D].  Prints rc / err, info, one `pair g1 g2 moving1 moving2 margin`
//       per table row and one `spair g1 g2 margin contact deep` per static-static pair; writes
//       out.contact and out.deep (bytes [N][P]), out.first (int32 [N]: chain_first_pair's column)
//       and out.contact_only (bytes [N][P]: the report without deep)
//   check_chain_report twin model.xml poses.bin out
//       a free-body model (strict loader); poses.bin: raw doubles [N][nq].  Per pose the model's qpos0
//       is replaced and scene_build run without movers: prints `spair g1 g2` per env-env pair, writes
//       out.contact and out.deep (bytes [N][pairs]: collide<false>'s and collide<true>'s counts)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "sspp_scene_build.h"
#include "sspp_chain_report.h"

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
    if (argc < 5) return 2;
    const std::string mode = argv[1];
    if (mode == "chain") {
        if (argc < 6) return 2;
        sspp_model m;
        if (report_rc(sspp::load_mjcf(argv[2], m, true))) return 0;
        const int D = std::atoi(argv[3]);
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
        for (const sspc::CStatic& s : t.statics)
            std::printf("spair %d %d %.17g %d %d\n", s.g1, s.g2, s.margin, (int)s.contact, (int)s.deep);
        const std::vector<double> q = read_doubles(argv[4]);
        const size_t N = q.size() / (size_t)D;
        std::vector<double> frames((size_t)7 * std::max(1, nd));
        // (0xee: an entry the routine leaves unwritten shows)
        std::vector<uint8_t> contact(N * (size_t)np, 0xee), deep(N * (size_t)np, 0xee), only(N * (size_t)np, 0xee);
        std::vector<int32_t> first(N, -2);
        for (size_t i = 0; i < N; ++i) {
            const double* qi = &q[i * D];
            const sspc::ArrayFrames fr{frames.data()};
            sspc::chain_fk(t.bodies.data(), t.joints.data(), nd, D, [qi](int adr) { return qi[adr]; }, fr);
            sspc::chain_pair_report(t.geoms.data(), t.pairs.data(), np, fr, contact.data() + i * np, deep.data() + i * np);
            sspc::chain_pair_report(t.geoms.data(), t.pairs.data(), np, fr, only.data() + i * np, (uint8_t*)nullptr);
            first[i] = sspc::chain_first_pair(t.geoms.data(), t.pairs.data(), np, fr);
        }
        const std::string out = argv[5];
        return write_raw(out + ".contact", contact) && write_raw(out + ".deep", deep) && write_raw(out + ".first", first) &&
                       write_raw(out + ".contact_only", only)
                   ? 0
                   : 7;
    }
    if (mode == "twin") {
        sspp_model m;
        if (report_rc(sspp::load_mjcf(argv[2], m, false))) return 0;
        const int nq = (int)m.qpos0.size();
        const std::vector<double> q = read_doubles(argv[3]);
        const size_t N = nq ? q.size() / (size_t)nq : 0;
        std::vector<uint8_t> contact, deep;
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
                deep.assign(N * P, 0);
            }
            if (t.statics.size() != P) return 8;
            for (size_t k = 0; k < P; ++k) {
                contact[i * P + k] = t.statics[k].contact;
                deep[i * P + k] = t.statics[k].deep;
            }
        }
        const std::string out = argv[4];
        return write_raw(out + ".contact", contact) && write_raw(out + ".deep", deep) ? 0 : 7;
    }
    return 2;
}
