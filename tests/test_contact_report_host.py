"""The contact report on the host, without a GPU: tests/contact_report/check_report.cpp fills an
sspp_model from arrays this test writes, runs the factored scene builder and the report's per-pose
routine (sspr::pose_report — the code the report kernels loop over) and prints pair infos, the
env-env pairs' counts and the [N][P] counts.  They are compared with tests/contact_report_ref.py:
exactly for oracle-type pairs, with at most MAX_NEAR near poses left out for the brute-force ones.
A second build of the same program runs under AddressSanitizer / UBSan (a stand-alone program).
Also: the new symbols and struct as sspp_amd/_lib.py binds them, and the name look-ups.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import mjcf_ref
from tests import capsule_scenes as CS
from tests import contact_report_ref as CRR
from tests import cylcyl_scenes as CC
from tests import synth_scenes as Y

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sspp_amd", "csrc")


def _build(out, extra=()):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "the host build needs hipcc"
    return subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-mfma",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), *extra,
                           os.path.join(HERE, "contact_report", "check_report.cpp"), "-o", out],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("contact_report") / "check_report")
    r = _build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


SAN_FLAGS = ["-g", "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    """the program under ASan / UBSan; skipped only when a one-line program cannot be built and run
    with the same flags (no sanitizer runtime) — check_report.cpp itself must then build"""
    d = tmp_path_factory.mktemp("contact_report_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "the host build needs hipcc"
    p = subprocess.run([hipcc, "-x", "hip", "--offload-host-only", *SAN_FLAGS, str(probe), "-o", str(d / "probe")],
                       capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime on this machine: " + (p.stderr.strip().splitlines() or ["probe failed"])[-1][:200])
    out = str(d / "check_report_san")
    r = _build(out, SAN_FLAGS)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def write_input(path, ref, mode, arg, qs):
    f = lambda v: " ".join(repr(float(x)) for x in np.asarray(v, float).reshape(-1))  # noqa: E731
    nb, ng = len(ref["body_parent"]), len(ref["geom_type"])
    bp, bq = np.asarray(ref["body_pos"], float).reshape(nb, 3), np.asarray(ref["body_quat"], float).reshape(nb, 4)
    gs, gp = np.asarray(ref["geom_size"], float).reshape(ng, 3), np.asarray(ref["geom_pos"], float).reshape(ng, 3)
    gq = np.asarray(ref["geom_quat"], float).reshape(ng, 4)
    out = ["%d %d" % (mode, arg), str(nb)]
    for b in range(nb):
        out.append("%d %d %d %s %s" % (ref["body_parent"][b], ref["body_jnt_type"][b], ref["body_qpos_adr"][b],
                                       f(bp[b]), f(bq[b])))
    out.append(str(ng))
    for g in range(ng):
        out.append("%d %d %d %d %s %s %s %s" % (ref["geom_type"][g], ref["geom_body"][g], ref["geom_contype"][g],
                                                ref["geom_conaffinity"][g], f(gs[g]), f(gp[g]), f(gq[g]),
                                                repr(float(ref["geom_margin"][g]))))
    ex = np.asarray(ref["exclude"], int).reshape(-1)
    out.append("%d %s" % (len(ex) // 2, " ".join(str(x) for x in ex)))
    out.append("%d %s" % (len(ref["qpos0"]), f(ref["qpos0"])))
    qs = np.asarray(qs, float)
    out.append("%d %d" % qs.shape)
    out += [f(q) for q in qs]
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


def run(exe, path, env=None):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = dict(pairs=[], spairs=[], contact=[], deep=[], stderr=r.stderr)
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "form":
            out["form"] = int(w[1])
        elif w[0] == "pair":
            out["pairs"].append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), float(w[5])))
        elif w[0] == "static":
            out["static"] = (int(w[1]), float(w[2]))
        elif w[0] == "spair":
            out["spairs"].append((int(w[1]), int(w[2]), float(w[3]), int(w[4]), int(w[5])))
        elif w[0] == "row":
            for key, h in (("contact", w[1]), ("deep", w[2])):
                out[key].append(np.frombuffer(bytes.fromhex("" if h == "-" else h), np.uint8))
    out["contact"], out["deep"] = np.array(out["contact"]), np.array(out["deep"])
    return out


def load(tmp, name, scene):
    """(mjcf_ref model, xml path) of a synthetic scene: an MJCF string or capsule_scenes' (statics, bodies)"""
    p = os.path.join(str(tmp), name + ".xml")
    with open(p, "w") as f:
        f.write(scene if isinstance(scene, str) else CS.mjcf(*scene, as_explicit=True))
    return mjcf_ref.load(p)


# (name, scene, mode, arg, pose seed, what the reference must show: multi, deep > contact, shallow).
# Seeds: the first of 1, 2, .. at which the reference alone shows everything the scene can show.
# deep > contact needs a box-box pair (every other collider counts its deep contacts among its
# contacts); two pairs touching at once needs statics closer together than the single-geom movers
# of the capsule and cylinder-cylinder scenes are wide.
SCENES = [
    ("zoo", Y.zoo, 0, 7, 1, (True, True, True)),
    ("two_movers", Y.two_movers, 0, 9, 1, (True, True, True)),
    # narrower qpos windows (the first mover's undriven entries come from the scene's defaults): dof 3
    # drives the position only, dof 6 leaves the quaternion's last entry at its default
    ("zoo_d3", Y.zoo, 0, 3, 3, (True, True, True)),
    ("zoo_d6", Y.zoo, 0, 6, 1, (True, True, True)),
    ("grid", lambda: Y.grid(3, 24), 0, 7, 2, (True, True, True)),
    ("tsp_boxes", Y.tsp_boxes, 1, "mover", 5, (True, True, True)),
    ("tsp_cylinders", lambda: Y.tsp_cylinders(True), 1, "mover", 1, (True, False, True)),
    ("capsule", CS.sspp_capsule_mover, 0, 7, 1, (False, False, True)),
    ("cylcyl", CC.sspp_cyl_mover, 0, 7, 1, (False, False, True)),
]


# touching / free poses every pair type must show (the issue's 4; the narrow windows turn the mover
# less or not at all, so their rarest type — sphere-sphere, plane-box — shows fewer in 257 poses)
MIN_EACH = {"zoo_d3": 2, "zoo_d6": 3}


def poses_for(ref, mode, arg, seed):
    return CRR.body_poses(seed) if mode == 1 else CRR.qpos_poses_d(arg, ref["qpos0"], seed)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """each scene's model, poses and reference, computed once"""
    tmp = tmp_path_factory.mktemp("contact_report_scenes")
    made = {}

    def get(name):
        if name not in made:
            _, scene, mode, arg, seed, want = next(s for s in SCENES if s[0] == name)
            ref = load(tmp, name, scene())
            if isinstance(arg, str):
                arg = ref["body_names"].index(arg)
            qs = poses_for(ref, mode, arg, seed)
            pairs = CRR.columns(ref, mode, arg)
            contact, deep, near = CRR.pair_counts(ref, mode, arg, pairs, qs)
            for a in (qs, contact, deep, near):
                a.setflags(write=False)
            made[name] = dict(ref=ref, mode=mode, arg=arg, qs=qs, pairs=pairs, contact=contact, deep=deep, near=near,
                              want=want, tmp=tmp)
        return made[name]

    return get


def check_case(exe, c, name, env=None):
    inp = os.path.join(str(c["tmp"]), name + ".in")
    write_input(inp, c["ref"], c["mode"], c["arg"], c["qs"])
    r = run(exe, inp, env)
    assert [(p[0], p[1]) for p in r["pairs"]] == c["pairs"]
    mv = set(CRR.moving_bodies(c["ref"], c["mode"], c["arg"]))
    for g1, g2, m1, m2, mg in r["pairs"]:
        assert (m1, m2) == (int(c["ref"]["geom_body"][g1] in mv), int(c["ref"]["geom_body"][g2] in mv))
        assert mg == max(c["ref"]["geom_margin"][g1], c["ref"]["geom_margin"][g2])
    keep = ~c["near"]
    assert c["near"].sum() <= CRR.MAX_NEAR
    np.testing.assert_array_equal(r["contact"][keep], c["contact"][keep])
    np.testing.assert_array_equal(r["deep"][keep], c["deep"][keep])
    return r


@pytest.mark.parametrize("name", [s[0] for s in SCENES])
def test_host_routine_against_reference(exe, cases, name):
    c = cases(name)
    multi, deep_gt, shallow = c["want"]
    types = CRR.assert_not_vacuous(c["ref"], c["pairs"], c["contact"], c["deep"], MIN_EACH.get(name, 4),
                                   want_multi=multi, want_deep_gt=deep_gt, want_shallow=shallow)
    if name.startswith("zoo"):
        assert types == [(0, 2), (0, 5), (0, 6), (2, 2), (2, 5), (2, 6), (5, 6), (6, 6)] and len(c["pairs"]) == 11
    if name == "zoo":
        assert c["contact"].max() == 4 and ((c["deep"] >= 5) & (c["contact"] == 1)).any()
    if name == "two_movers":
        gb = c["ref"]["geom_body"]
        assert len(c["pairs"]) == 12 and any(gb[a] != 0 and gb[b] != 0 for a, b in c["pairs"])  # mover-mover
    if name == "grid":
        assert len(c["pairs"]) == 72
    if name in ("capsule", "cylcyl"):
        assert not c["near"].all()
    r = check_case(exe, c, name)
    # no env-env pair in these worlds but two_movers' (none): the sums are empty
    assert r["static"][0] == sum(p[3] for p in r["spairs"])


def test_static_contact_world(exe, tmp_path):
    """capsule_scenes' env-env world: the resting capsule and its tray, one contact; the per-pair
    counts sum to static_contacts and equal the reference's."""
    ref = load(tmp_path, "static_contact", CS.sspp_static_contact())
    qs = CRR.qpos_poses(1, 8)
    inp = str(tmp_path / "static.in")
    write_input(inp, ref, 0, 7, qs)
    r = run(exe, inp)
    names = ref["geom_names"]
    want = CRR.static_counts(ref, 0, 7)
    assert [(a, b, c, d) for a, b, _, c, d in r["spairs"]] == want
    touching = [(names[a], names[b], c) for a, b, _, c, d in r["spairs"] if c]
    assert touching == [("tray", "pin", 1)]
    assert r["static"][0] == sum(p[3] for p in r["spairs"]) == 1


def test_host_routine_under_sanitizers(exe, exe_san, cases):
    """The same program with -fsanitize=address,undefined, run as a program on the zoo and the
    two-mover scene: clean, and the same bytes as the plain build."""
    for name in ("zoo", "zoo_d3", "two_movers", "tsp_boxes"):
        c = cases(name)
        r = check_case(exe_san, c, name)
        assert "runtime error" not in r["stderr"] and "AddressSanitizer" not in r["stderr"], r["stderr"][-2000:]
        p = check_case(exe, c, name)
        assert np.array_equal(r["contact"], p["contact"]) and np.array_equal(r["deep"], p["deep"])


# ------------------------------------------------------------------ ABI
def test_abi_symbols_and_struct():
    from sspp_amd import _lib
    L = _lib.lib()
    new = ["sspp_scene_pairs", "sspp_scene_static_pairs", "sspp_model_geom_name", "sspp_model_body_name",
           "sspp_scene_contacts", "sspp_job_path_contacts"]
    declared = _lib.declared_symbols()
    for s in new:
        assert s in declared and s in _lib.SIGNATURES and hasattr(L, s), s
    assert C.sizeof(_lib.PairInfo) == 24
    assert [f[0] for f in _lib.PairInfo._fields_] == ["geom1", "geom2", "moving1", "moving2", "margin"]
    assert _lib.PairInfo.margin.offset == 16
    txt = open(_lib.HEADER_PATH).read()
    m = re.search(r"typedef struct sspp_pair_info \{(.*?)\} sspp_pair_info;", txt, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(int32_t|double)\s+([^;]+);", body) == [("int32_t", "geom1, geom2"),
                                                                 ("int32_t", "moving1, moving2"), ("double", "margin")]


def test_names_round_trip():
    import sspp_amd as S
    from sspp_amd import _lib
    m = S.Model(os.path.join(S.SCENE_DIR, "robocrane.xml"))
    a = m.arrays()
    ng, nb = len(a["geom_type"]), len(a["body_parent"])
    named = 0
    for g in range(ng):
        n = m.geom_name(g)
        if n:
            named += 1
            assert m.geom_id(n) == g
    assert named > 10
    for b in range(nb):
        n = m.body_name(b)
        if n:
            assert m.body_id(n) == b
    assert m.body_name(m.body_id("blockwall1")) == "blockwall1"
    L = _lib.lib()
    for bad in (-1, ng):
        assert L.sspp_model_geom_name(m.handle, bad) is None
    for bad in (-1, nb):
        assert L.sspp_model_body_name(m.handle, bad) is None
