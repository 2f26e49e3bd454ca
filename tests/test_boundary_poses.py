"""The boundary-pose generator (tests/boundary_poses.py) checked from the reference alone, and the
host build of the device narrowphase (sspd::collide's variants, sspd::pair_near) on its poses.

Every pose lies touch(d) + off along its case's approach direction.  For |off| >= 1e-9 the
reference must report contact (or deep contact) exactly when off < 0: a condition, with no pose
left out.  Every pair type meets that floor, the cylinder-box root searches included
(boundary_poses.FLOORS is empty).  Where the touching distance has a closed form the bisected one
equals it within 1e-12, which ties the set to geometry and not only to the oracle.  The
SamplingPathPlanner cases the oracle decides also carry the bisection's two ends (off = -0.0 /
+0.0, one rounding step apart): the only poses close enough for the culls' 1e-9 pad to matter —
with kHullPad removed the host check below fails on one such pose of the box scene at margin 1e-2.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import boundary_poses as BP
from tests import capsule_scenes as CS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
PAIR_TYPES = {"plane-sphere", "plane-cylinder", "plane-box", "sphere-sphere", "sphere-cylinder", "sphere-box",
              "cylinder-box", "box-box", "plane-capsule", "sphere-capsule", "capsule-capsule", "capsule-box"}
# which side of a mixed pair moves, per scene kind: every role the loader and the scene builder
# permit (a plane has no free body; a capsule-cylinder pair is refused)
ROLES = {"plane-sphere": {"sphere"}, "plane-cylinder": {"cylinder"}, "plane-box": {"box"}, "plane-capsule": {"capsule"},
         "sphere-sphere": {"sphere"}, "sphere-cylinder": {"sphere", "cylinder"}, "sphere-box": {"sphere", "box"},
         "sphere-capsule": {"sphere", "capsule"}, "cylinder-box": {"cylinder", "box"}, "box-box": {"box"},
         "capsule-capsule": {"capsule"}, "capsule-box": {"capsule", "boxcap"}}


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("boundary_poses"))


def all_sets(root):
    """(label, ref, cases, poses, deep) of every scene, margin and threshold."""
    for kind in BP.SSPP_KINDS:
        for margin in BP.MARGINS:
            yield ("sspp %s margin %g" % (kind, margin), kind) + BP.sspp_set(root, kind, margin) + (False,)
    for name in BP.TSP_SCENES:
        for deep in (False, True):
            yield ("tsp %s %s" % (name, "deep" if deep else "contact"), "box") + BP.tsp_set(root, name, deep) + (deep,)


@pytest.fixture(scope="module")
def decisions(root):
    """The reference's (contacts, deep contacts) at every pose of every set, computed once."""
    out = {}
    for label, kind, ref, cases, P, deep in all_sets(root):
        r = np.array([ref.contacts(q) for q in P["q"]])
        r.setflags(write=False)
        out[label] = (kind, ref, cases, P, deep, r)
    return out


def test_offsets_are_the_issue_list():
    mags = sorted({abs(o) for o in BP.OFFSETS})
    assert mags == [1e-12, 1e-9, 1e-7, 1e-6, 1e-5, 5e-5, 1e-4, 2e-4, 3e-4, 1e-3]
    assert sorted(BP.OFFSETS) == sorted([-m for m in mags] + mags)
    # the filter's eps = 2e-4 m (S <= 1 in these scenes) and its 6e-5 error bound are straddled
    assert any(6e-5 < m < 2e-4 for m in mags) and any(m < 6e-5 for m in mags) and any(m > 2e-4 for m in mags)
    assert BP.FLOOR == 1e-9 and BP.FLOORS == {}


def test_decision_follows_the_offset_sign(decisions):
    """Contact (deep contact for the deep sets) exactly when off < 0, for every pose with
    |off| >= the floor; every pair type, family, margin and threshold shows both outcomes."""
    seen = {}
    total = 0
    for label, (kind, ref, cases, P, deep, r) in decisions.items():
        assert len(P["q"]) == sum(len(BP.offsets_of(c)) for c in cases)
        hit = r[:, 1 if deep else 0] > 0
        for i, (off, k) in enumerate(zip(P["off"], P["case"])):
            c = cases[k]
            total += 1
            if off == 0.0:   # the bisection's ends: touching at -0.0, clear at +0.0, by construction
                assert hit[i] == bool(np.signbit(off)), (label, c["pair"], c["feature"], off)
                continue
            if abs(off) < BP.FLOORS.get(c["pair"], BP.FLOOR):
                continue
            assert hit[i] == (off < 0), (label, c["pair"], c["feature"], c["family"], off, r[i])
            for key in (("pair", c["pair"]), ("family", c["family"]), ("set", label), ("pair-set", c["pair"], label),
                        ("role", c["pair"], kind)):
                seen.setdefault(key, set()).add(bool(hit[i]))
    assert all(v == {True, False} for v in seen.values())
    assert {k[1] for k in seen if k[0] == "pair"} == PAIR_TYPES
    assert {k[1] for k in seen if k[0] == "family"} == set("abcde")
    for pair, kinds in ROLES.items():
        assert {k[2] for k in seen if k[0] == "role" and k[1] == pair} >= kinds, pair
    assert 3000 <= total <= 20000


def test_only_the_target_decides(decisions):
    """A pose's contacts are its target pair's alone: without the target static nothing is left."""
    from oracle import oracle as O
    from tests import synth_scenes as Y
    for label, (kind, ref, cases, P, deep, r) in decisions.items():
        if ref.has_capsule:
            continue   # (the composed reference has no per-geom switch; the pair rows below cover it)
        for k, c in enumerate(cases):
            rows = np.flatnonzero(P["case"] == k)
            sc = O.Scene(Y.with_geoms_off(ref.ref, [ref.geom(c["target"])]), ref.mode, ref.arg)
            assert all(sc.contacts(P["q"][i])[0] == 0 for i in rows[::5]), (label, c["target"])


def test_families_reach_their_branches(root):
    ref, cases, P = BP.sspp_set(root, "box", 0.0)
    fam = {f: [c for c in cases if c["family"] == f] for f in "abcde"}
    assert all(len(v) >= 3 for v in fam.values())
    for c in fam["a"]:
        assert np.array_equal(CS.quat2mat(c["quat"]), np.eye(3).ravel())
    for c in fam["b"]:   # upright3's exact zeros, and a genuine yaw
        m = CS.quat2mat(c["quat"])
        assert m[2] == 0.0 and m[5] == 0.0 and m[6] == 0.0 and m[7] == 0.0 and m[1] != 0.0
    # (d) box-box on an upright static: the edge axes |A_i x B_j| on both sides of the FP64 cut
    # |L| = 1e-6, some inside the filter's band (sqrt(kLenEval2) = 2.1e-5), upright3 just off
    lens = []
    for c in fam["d"]:
        if c["pair"] != "box-box" or c["target"] not in ("box_up", "box_yaw"):
            continue
        A, Bm = BP.ref_mat(ref, c["target"]), BP.rot(c["quat"])
        m = Bm.ravel()
        assert not (m[2] == 0.0 and m[5] == 0.0 and m[6] == 0.0 and m[7] == 0.0)
        L = [np.linalg.norm(np.cross(A[:, i], Bm[:, j])) for i in range(3) for j in range(3)]
        lens.append(min(x for x in L if x > 1e-9))
    lens = np.array(lens)
    assert len(lens) >= 10 and (lens < 1e-6).sum() >= 2 and ((lens > 1e-6) & (lens < 2.1e-5)).sum() >= 2 and (lens > 2.1e-5).any()
    n2 = np.array([c["quat"] @ c["quat"] for c in fam["e"]])
    assert (n2 < 0.25).any() and (n2 > 0.25).any() and np.allclose(np.sort(np.unique(np.round(n2, 12))), [0.2, 0.3])
    # every other scene carries an unnormalised row too
    for kind in BP.SSPP_KINDS[1:]:
        assert any(c["family"] == "e" for c in BP.sspp_set(root, kind, 0.0)[1]), kind


def test_closed_form_touching_distances(root):
    """Sphere-sphere, plane-sphere, plane-box, face-face boxes and a sphere over a box face: the
    bisected touch(d) against its closed form, within 1e-12, at every margin."""
    seen = set()
    for kind in BP.SSPP_KINDS:
        for margin in BP.MARGINS:
            ref, cases, P = BP.sspp_set(root, kind, margin)
            for k, c in enumerate(cases):
                if c["closed"] is None:
                    continue
                want = c["closed"](margin, c, ref)
                assert abs(P["touch"][k] - want) <= 1e-12, (kind, margin, c["pair"], c["feature"], c["family"], P["touch"][k], want)
                seen.add((c["pair"], c["feature"]))
    assert seen >= {("sphere-sphere", "point"), ("plane-sphere", "point"), ("plane-box", "corner"), ("box-box", "face-face"),
                    ("sphere-box", "face")}


def test_scene_tables(root):
    """Targets at least 2 m apart, everything within 8 m, and the three table sizes: fewer than
    9 pairs, 12 and 65, counted by the oracle; the filler statics never touch (the big table's
    decisions are the small table's)."""
    for kind in BP.SSPP_KINDS:
        st, _ = BP.sspp_scene(kind, 0.0, "small")
        pos = np.array([g["pos"] for g in st if g["type"] != BP.PLANE])
        for i in range(len(pos)):
            for j in range(i):
                assert np.linalg.norm(pos[i] - pos[j]) >= 2.0
        ref, cases, P = BP.sspp_set(root, kind, 0.0)
        assert np.abs(P["q"][:, :3]).max() <= 8.0
        counts = {}
        for table in BP.TABLES:
            stt, bodies = BP.sspp_scene(kind, 0.0, table)
            assert max(np.abs(g["pos"]).max() for g in stt) <= 8.0
            _, ref_path = BP.write_scene(root, "tab_%s_%s" % (kind, table), (stt, bodies))
            r2 = BP.Ref(ref_path, 0, 7)
            counts[table] = r2.full.npairs()[0]
            if table == "big":
                sub = range(0, len(P["q"]), 7)
                assert all(r2.contacts(P["q"][i]) == ref.contacts(P["q"][i]) for i in sub)
        assert counts["small"] < 9 and counts["hull"] == 12 and counts["big"] == 65, counts


# ------------------------------------------------------------------ host build of the device code
def hexrow(*parts):
    return " ".join(float(x).hex() for p in parts for x in np.ravel(p))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs_host")
    exe = str(d / "check_pairs")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "the host build of the device code needs hipcc"
    subprocess.check_call([hipcc, "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "sspp_amd", "csrc"),
                           os.path.join(HERE, "narrowphase", "check_pairs.cpp"), "-o", exe])

    def run(rows):
        path = str(d / "cases.txt")
        with open(path, "w") as f:
            f.write("\n".join(rows) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out = np.array([[int(x) for x in line.split()] for line in r.stdout.splitlines()])
        assert out.shape == (len(rows), 6)
        return out

    return run


def pair_row(ref, c, q):
    """The target pair of a pose as sspd::collide takes it: geom 1 first by (type, index)."""
    xp, xm = ref.full.fk(q)
    gm, gt = ref.geom("m_geom"), ref.geom(c["target"])
    ty, size, mg = ref.ref["geom_type"], np.asarray(ref.ref["geom_size"], float), ref.ref["geom_margin"]
    a, b = (gm, gt) if (ty[gm], gm) < (ty[gt], gt) else (gt, gm)
    return hexrow([ty[a], ty[b], max(mg[gm], mg[gt])], xp[a], xm[a], size[a], xp[b], xm[b], size[b], [1 if a == gm else 2])


def test_host_narrowphase_on_boundary_poses(decisions, host_check):
    """sspd::collide<false> / <true> and the TaskSpacePlanner kernels' variants (CB = 2, OUTLINE,
    UP, wherever their precondition holds) on every pose, |off| = 1e-12 included: the variants
    agree with each other and, behind pair_near, with the reference's contact and deep counts.
    pair_near never culls a pose the reference reports in contact.  (With a margin the SAT alone
    reports corner-to-corner boxes in contact whose bounding spheres the broadphase separates: the
    reference's answer there is the cull's, and the comparison is made behind pair_near.)"""
    ran = {"cb2": 0, "up": 0, "culled": 0, "sat_only": 0}
    for label, (kind, ref, cases, P, deep, r) in decisions.items():
        got = host_check([pair_row(ref, cases[k], q) for q, k in zip(P["q"], P["case"])])
        nc, nd, cb2, outl, up, near = got.T
        np.testing.assert_array_equal(np.where(near == 1, nc, 0), r[:, 0], err_msg=label)
        np.testing.assert_array_equal(np.where(near == 1, nd, 0), r[:, 1], err_msg=label)
        assert (near[r[:, 0] > 0] == 1).all(), label
        np.testing.assert_array_equal(outl, nd, err_msg=label)
        assert (cb2[cb2 >= 0] == nd[cb2 >= 0]).all() and (up[up >= 0] == nd[up >= 0]).all(), label
        pairs = np.array([cases[k]["pair"] for k in P["case"]])
        ran["cb2"] += int(((cb2 >= 0) & (pairs == "cylinder-box")).sum())
        ran["up"] += int(((up >= 0) & (pairs == "box-box")).sum())
        ran["culled"] += int((near == 0).sum())
        ran["sat_only"] += int(((near == 0) & (nc > 0)).sum())
    assert ran["cb2"] >= 100 and ran["up"] >= 100 and ran["culled"] >= 100 and ran["sat_only"] >= 1, ran


def test_host_sphere_centre_inside_box(host_check):
    """The sphere-box rule with the centre inside the box (dist <= -r, away from every threshold):
    one contact, deep, in every variant."""
    eye = np.eye(3).ravel()
    rows = [hexrow([BP.SPHERE, BP.BOX, m], c, eye, [r, 0, 0], [0, 0, 0], eye, e, [1])
            for r, e, c in BP.SPHERE_INSIDE for m in BP.MARGINS]
    got = host_check(rows)
    assert (got == 1).all()
