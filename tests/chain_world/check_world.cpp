// Host-only run of the worlds of arms (tests/test_chain_world_host.py, tests/test_gpu_chain_world.py):
// the MJCF loader, sspc::chain_build with a world, the updates' host half (chain_world_qpos /
// chain_world_body_pose on a trial copy, chain_update, adopt: what sspp_chain_set_qpos /
// _set_body_pose do before they copy the tables to the device) and the per-pose routines the chain
// kernels loop over.  No GPU.
//
//   check_world run model.xml D count_static ops.txt poses.bin out
//       ops.txt, one per line, applied in order to a chain at the model's own world:
//         qpos N v0 .. v(N-1)             sspp_chain_set_qpos's host half
//         body ID px py pz qw qx qy qz    sspp_chain_set_body_pose's host half
//         rawqpos N v0 ..                 the values written into the world as they are
//         rawbody ID px py pz qw qx qy qz the values written into body_pos / body_quat as they are
//       (raw ops edit the model data directly: chain_build then runs once, after the last op, on
//       model data holding the new values).  Per product op prints `op RC EPOCH HASH` (HASH: FNV-1a
//       of the table bytes after the op) and `err MESSAGE` on a failure; then `rc`, `info`, one
//       `pair g1 g2 moving1 moving2 margin` per table row, one `spair g1 g2 margin contact deep` per
//       static pair, `epoch`, `hash`, `qpos v..` (the world).
//       poses.bin: raw doubles [N][D].  Writes out.tables (the body, joint, geom and pair records'
//       bytes), out.fk ([N][ngeom][3 + 9]), out.hit (N bytes, static block included), out.contact and
//       out.deep ([N][pairs] counts), out.first (int32 [N]: the lowest column in contact, -1 none)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
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
template <class T>
void append_bytes(std::vector<uint8_t>& to, const std::vector<T>& v) {
    const uint8_t* p = (const uint8_t*)v.data();
    to.insert(to.end(), p, p + v.size() * sizeof(T));
}
std::vector<uint8_t> table_bytes(const sspc::ChainTables& t) {
    std::vector<uint8_t> b;
    append_bytes(b, t.bodies);
    append_bytes(b, t.joints);
    append_bytes(b, t.geoms);
    append_bytes(b, t.pairs);
    return b;
}
unsigned long long fnv(const std::vector<uint8_t>& b) {
    unsigned long long h = 1469598103934665603ull;
    for (uint8_t x : b) h = (h ^ x) * 1099511628211ull;
    return h;
}
}  // namespace
int sspp::set_error(int code, const std::string& msg) { g_err = msg; return code; }
void sspp::clear_error() { g_err.clear(); }

int main(int argc, char** argv) {
    if (argc < 8 || std::string(argv[1]) != "run") return 2;
    sspp_model base;
    int rc = sspp::load_mjcf(argv[2], base, true);
    std::printf("rc %d\n", rc);
    if (rc) { std::printf("err %s\n", g_err.c_str()); return 0; }
    const int D = std::atoi(argv[3]), count_static = std::atoi(argv[4]);
    // the chain: its own copy of the model data, its world, its tables, its epoch
    sspp_model model = base;
    std::vector<double> world = base.qpos0;
    sspc::ChainTables t;
    long long epoch = 0;
    rc = sspc::chain_build(model, D, t);
    if (rc) { std::printf("rc %d\nerr %s\n", rc, g_err.c_str()); return 0; }
    bool raw = false;
    std::ifstream ops(argv[5]);
    std::string line;
    while (std::getline(ops, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        const bool product = kind == "qpos" || kind == "body";
        sspp_model trial = model;
        std::vector<double> w = world;
        int orc = SSPP_OK;
        g_err.clear();
        if (kind == "qpos" || kind == "rawqpos") {
            int n = 0;
            in >> n;
            std::vector<double> v((size_t)std::max(n, 0));
            for (double& x : v) {
                std::string tok;
                in >> tok;
                x = std::strtod(tok.c_str(), nullptr);  // (nan and inf included)
            }
            if (product) orc = sspc::chain_world_qpos(model, v.data(), n, "sspp_chain_set_qpos", w);
            else w = v;
        } else if (kind == "body" || kind == "rawbody") {
            int id = 0;
            double p[3], q[4];
            in >> id;
            for (double& x : p) { std::string tok; in >> tok; x = std::strtod(tok.c_str(), nullptr); }
            for (double& x : q) { std::string tok; in >> tok; x = std::strtod(tok.c_str(), nullptr); }
            if (product) orc = sspc::chain_world_body_pose(trial, w, id, p, q);
            else {
                for (int k = 0; k < 3; ++k) trial.body_pos[3 * id + k] = p[k];
                for (int k = 0; k < 4; ++k) trial.body_quat[4 * id + k] = q[k];
            }
        } else
            return 3;
        if (product) {
            sspc::ChainTables nt;
            if (!orc) orc = sspc::chain_update(t, trial, w, nt);
            if (!orc) {
                t = std::move(nt);
                model = std::move(trial);
                world = std::move(w);
                ++epoch;
            }
            std::printf("op %d %lld %llu\n", orc, epoch, fnv(table_bytes(t)));
            if (orc) std::printf("err %s\n", g_err.c_str());
        } else {
            model = std::move(trial);
            world = std::move(w);
            raw = true;
        }
    }
    if (raw) {  // model data holding the new values: one build
        rc = sspc::chain_build(model, D, t, world.data());
        if (rc) { std::printf("rc %d\nerr %s\n", rc, g_err.c_str()); return 0; }
    }
    const int nd = (int)t.bodies.size(), ng = (int)t.geoms.size(), np = (int)t.pairs.size();
    std::printf("info %d %d %d %d %d %d %d\n", nd, ng, t.n_moving_geoms, t.n_static_geoms, np, t.n_static_pairs,
                t.static_contacts);
    for (const sspc::CPair& p : t.pairs) {
        const int g1 = std::min(p.a, p.b), g2 = std::max(p.a, p.b);
        std::printf("pair %d %d %d %d %.17g\n", g1, g2, (int)(t.geoms[g1].slot >= 0), (int)(t.geoms[g2].slot >= 0), p.margin);
    }
    for (const sspc::CStatic& s : t.statics) std::printf("spair %d %d %.17g %d %d\n", s.g1, s.g2, s.margin, s.contact, s.deep);
    std::printf("epoch %lld\nhash %llu\nqpos", epoch, fnv(table_bytes(t)));
    for (double v : world) std::printf(" %.17g", v);
    std::printf("\n");
    const std::vector<double> q = read_doubles(argv[6]);
    const size_t N = q.size() / (size_t)D;
    const int static_block = (count_static && t.static_contacts > 0) ? 1 : 0;
    std::vector<double> fk(N * (size_t)ng * 12), frames((size_t)7 * std::max(1, nd));
    std::vector<uint8_t> hit(N), contact(N * (size_t)np), deep(N * (size_t)np), row((size_t)std::max(1, np));
    std::vector<int32_t> first(N);
    for (size_t i = 0; i < N; ++i) {
        const double* qi = &q[i * D];
        const sspc::ArrayFrames fr{frames.data()};
        sspc::chain_fk(t.bodies.data(), t.joints.data(), nd, D, [qi](int adr) { return qi[adr]; }, fr);
        for (int g = 0; g < ng; ++g) {
            double* o = &fk[(i * ng + g) * 12];
            sspc::geom_pose(t.geoms.data() + g, fr, o, o + 3);
        }
        hit[i] = (uint8_t)((sspc::chain_contact(t.geoms.data(), t.pairs.data(), np, fr) || static_block) ? 1 : 0);
        if (np) sspc::chain_pair_report(t.geoms.data(), t.pairs.data(), np, fr, &contact[i * np], &deep[i * np]);
        first[i] = sspc::chain_first_pair(t.geoms.data(), t.pairs.data(), np, fr);
    }
    const std::string out = argv[7];
    const bool ok = write_raw(out + ".tables", table_bytes(t)) && write_raw(out + ".fk", fk) && write_raw(out + ".hit", hit) &&
                    write_raw(out + ".contact", contact) && write_raw(out + ".deep", deep) && write_raw(out + ".first", first);
    return ok ? 0 : 7;
}
