"""Articulated movers on the host, without a GPU: tests/chain/check_chain.cpp runs the MJCF loader
with hinge / slide joints, sspc::chain_build and the per-pose routines sspc::chain_fk / geom_pose /
chain_contact (sspp_chain.h: the code the chain kernels loop over).  Checked against closed forms
and against tests/chain_ref.py (numpy, written from the rule, no product code); pair types that
tests/capsule_ref.py does not decide go through the frozen twin (every link a free body at the
reference's pose, the scene builder's env-env path).  A second build of the same program runs under
AddressSanitizer / UBSan (a stand-alone program).
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import chain_host as H
from tests import chain_ref as R
from tests import chain_scenes as S


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chain") / "check_chain")
    r = H.build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    """the program under ASan / UBSan; skipped only when a one-line program cannot be built and run
    with the same flags (no sanitizer runtime) — check_chain.cpp itself must then build"""
    d = tmp_path_factory.mktemp("chain_san")
    why = H.sanitizer_probe(d)
    if why:
        pytest.skip("no sanitizer runtime on this machine: " + why)
    out = str(d / "check_chain_san")
    r = H.build(out, H.SAN_FLAGS)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def world_xml(tmp, name, world):
    return H.write_xml(tmp, name, S.mjcf(world))


# ------------------------------------------------------------------ loader
LOADER_XML = """<mujoco>
  <default>
    <joint axis="0 2 0" pos="0.1 0 0"/>
    <default class="rail"><joint type="slide" axis="3 0 4" ref="0.25"/></default>
    <default class="wrist"><joint ref="90" damping="3"/></default>
  </default>
  <worldbody>
    <body name="base" pos="0 0 0.2"><freejoint name="root"/>
      <geom name="bg" type="box" size="0.1 0.1 0.05"/>
      <body name="a" pos="0 0 0.1">
        <joint name="a1" range="-1 1" limited="true"/>
        <joint name="a2" type="hinge" axis="0 0 1" pos="0 0 0" ref="-45"/>
        <geom name="ag" type="capsule" size="0.03 0.1"/>
        <body name="b" pos="0 0 0.3" childclass="rail">
          <joint name="b1"/>
          <geom name="bgm" type="sphere" size="0.03"/>
          <body name="c" pos="0 0 0.1">
            <joint name="c1" class="wrist"/>
            <joint name="c2" type="hinge"/>
            <geom name="cg" type="sphere" size="0.02"/>
          </body>
        </body>
      </body>
    </body>
    <body name="fixed" pos="1 0 0"><geom name="fg" type="sphere" size="0.1"/></body>
  </worldbody>
</mujoco>
"""


def test_loader_joints(exe, tmp_path):
    """defaults and childclass on joints, ref in degrees, a non-unit axis, pos, two joints on one
    body, qpos addresses after a free base; the strict loader still refuses the file"""
    xml = H.write_xml(tmp_path, "loader", LOADER_XML)
    o = H.load(exe, xml)
    assert o["rc"] == 0, o["err"]
    assert o["nq"] == 7 + 5
    J = o["joints"]
    # c2: type="hinge" explicit under childclass rail (the class gives the axis and the ref, in degrees for a hinge)
    assert [(j[0], j[1], j[2], j[5]) for j in J] == [(0, 1, 0, "root"), (3, 2, 7, "a1"), (3, 2, 8, "a2"), (2, 3, 9, "b1"),
                                                     (3, 4, 10, "c1"), (3, 4, 11, "c2")]
    np.testing.assert_allclose(J[5][3], (0.6, 0, 0.8), atol=1e-16)
    np.testing.assert_allclose(J[1][3], (0, 1, 0), atol=0)         # main default axis 0 2 0, normalised
    np.testing.assert_allclose(J[1][4], (0.1, 0, 0), atol=0)       # main default pos
    np.testing.assert_allclose(J[2][3], (0, 0, 1), atol=0)
    np.testing.assert_allclose(J[2][4], (0, 0, 0), atol=0)
    np.testing.assert_allclose(J[3][3], (0.6, 0, 0.8), atol=1e-16)  # class rail: 3 0 4 normalised
    np.testing.assert_allclose(J[3][4], (0.1, 0, 0), atol=0)       # inherited from main
    np.testing.assert_allclose(J[4][3], (0, 1, 0), atol=0)         # class wrist inherits main's axis
    q0 = o["qpos0"]
    np.testing.assert_allclose(q0[:7], (0, 0, 0.2, 1, 0, 0, 0), atol=0)
    assert q0[7] == 0.0 and q0[8] == -45 * np.pi / 180.0
    assert q0[9] == 0.25                                            # a slide's ref: metres
    assert q0[10] == 90 * np.pi / 180.0
    assert q0[11] == 0.25 * np.pi / 180.0                           # class rail's ref on a hinge: degrees
    # body_jnt_type / body_qpos_adr report the first joint; the jointless body -1
    assert [b[:2] for b in o["bodies"]] == [(-1, -1), (0, 0), (3, 7), (2, 9), (3, 10), (-1, -1)]
    assert [b[2:] for b in o["bodies"]] == [(0, 0), (0, 1), (1, 2), (3, 1), (4, 2), (6, 0)]
    strict = H.load(exe, xml, joints=False)
    assert strict["rc"] == -5 and "unsupported joint type" in strict["err"]


def test_loader_radian_and_errors(exe, tmp_path):
    body = '<body name="b"><joint name="j" %s/><geom type="sphere" size="0.1"/></body>'
    wrap = lambda comp, b: "<mujoco>%s<worldbody>%s</worldbody></mujoco>" % (comp, b)  # noqa: E731
    o = H.load(exe, H.write_xml(tmp_path, "rad", wrap('<compiler angle="radian"/>', body % 'ref="0.5"')))
    assert o["rc"] == 0 and o["qpos0"][0] == 0.5
    o = H.load(exe, H.write_xml(tmp_path, "deg", wrap("", body % 'ref="0.5"')))
    assert o["rc"] == 0 and o["qpos0"][0] == 0.5 * np.pi / 180.0
    o = H.load(exe, H.write_xml(tmp_path, "ball", wrap("", body % 'type="ball"')))
    assert o["rc"] == -5 and "ball" in o["err"]
    o = H.load(exe, H.write_xml(tmp_path, "zero", wrap("", body % 'axis="0 0 0"')))
    assert o["rc"] == -3 and "zero axis" in o["err"]
    mixed = '<body name="b"><freejoint/><joint name="j"/><geom type="sphere" size="0.1"/></body>'
    o = H.load(exe, H.write_xml(tmp_path, "mixed", wrap("", mixed)))
    assert o["rc"] == -3 and "mixed" in o["err"]
    mixed2 = '<body name="b"><joint name="j"/><freejoint/><geom type="sphere" size="0.1"/></body>'
    o = H.load(exe, H.write_xml(tmp_path, "mixed2", wrap("", mixed2)))
    assert o["rc"] == -3 and "mixed" in o["err"]


def test_library_surface(tmp_path):
    """the library's loaders and getter as sspp_amd binds them: Model(joints=True).joints(), the
    strict Model still (-5), arrays() unchanged in its keys, Scene(model) (-5) naming the joint and
    the chain entry point (checked before any device call)"""
    import sspp_amd as A
    from sspp_amd import _lib
    xml = H.write_xml(tmp_path, "loader", LOADER_XML)
    with pytest.raises(A.SsppError, match=r"\(-5\).*unsupported joint type"):
        A.Model(xml)
    m = A.Model(xml, joints=True)
    j = m.joints()
    assert list(j["jnt_type"]) == [0, 3, 3, 2, 3, 3] and list(j["jnt_qpos_adr"]) == [0, 7, 8, 9, 10, 11]
    assert list(j["jnt_body"]) == [1, 2, 2, 3, 4, 4] and j["jnt_names"] == ["root", "a1", "a2", "b1", "c1", "c2"]
    np.testing.assert_allclose(j["jnt_axis"][3], (0.6, 0, 0.8), atol=1e-16)
    a = m.arrays()
    assert sorted(a) == sorted(["body_parent", "body_jnt_type", "body_qpos_adr", "body_pos", "body_quat", "geom_type",
                                "geom_body", "geom_contype", "geom_conaffinity", "geom_size", "geom_pos", "geom_quat",
                                "geom_margin", "exclude", "qpos0"])
    assert list(a["body_jnt_type"]) == [-1, 0, 3, 2, 3, -1] and len(a["qpos0"]) == 12
    with pytest.raises(A.SsppError, match=r"\(-5\).*'a1'.*sspp_chain_create"):
        A.Scene(m, A._lib.MODE_QPOS, 7)
    with pytest.raises(A.SsppError, match=r"\(-5\).*'a1'.*sspp_chain_create"):
        A.Scene(m, A._lib.MODE_BODY, "base")
    # a free-body file through the joint-accepting loader is the same model
    p = os.path.join(A.SCENE_DIR, "robocrane.xml")
    a0, a1 = A.Model(p).arrays(), A.Model(p, joints=True).arrays()
    assert all(np.array_equal(a0[k], a1[k]) for k in a0)
    assert set(A.Model(p, joints=True).joints()["jnt_type"]) == {0}
    declared = _lib.declared_symbols()
    for s in ("sspp_model_load_mjcf_joints", "sspp_model_joints_get", "sspp_chain_create", "sspp_chain_free",
              "sspp_chain_get_info", "sspp_chain_pairs", "sspp_chain_fk", "sspp_chain_contacts",
              "sspp_chain_score_ctrl", "sspp_chain_sample_score"):
        assert s in declared and s in _lib.SIGNATURES and hasattr(_lib.lib(), s), s
    assert C.sizeof(_lib.ChainInfo) == 32 and C.sizeof(_lib.JointView) == 64


# ------------------------------------------------------------------ FK, closed forms
def geom_fk(exe, tmp, name, world, D, q):
    o = H.chain(exe, world_xml(tmp, name, world), D, q, tmp, tag=name)
    assert o["rc"] == 0, o["err"]
    return o


def rotm(axis, a):
    x, y, z = axis
    c, s = np.cos(a), np.sin(a)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], float)
    return np.eye(3) + s * K + (1 - c) * (K @ K)


TOL = 1e-14  # closed forms against FP64 kinematics of a metre-scale arm: a few ulp of 1


def test_fk_planar_2r(exe, tmp_path):
    l1, l2 = 0.4, 0.3
    q = np.array([[0.0, 0.0], [0.3, -1.1], [2.5, 0.7], [-1.2, 3.0], [np.pi / 2, np.pi / 2]])
    o = geom_fk(exe, tmp_path, "planar", S.planar_2r(l1, l2), 2, q)
    elbow, tip = o["fk"][:, 0, :3], o["fk"][:, 1, :3]
    np.testing.assert_allclose(elbow, np.stack([l1 * np.cos(q[:, 0]), l1 * np.sin(q[:, 0]), 0.5 + 0 * q[:, 0]], 1), atol=TOL)
    s = q[:, 0] + q[:, 1]
    np.testing.assert_allclose(tip, np.stack([l1 * np.cos(q[:, 0]) + l2 * np.cos(s), l1 * np.sin(q[:, 0]) + l2 * np.sin(s),
                                              0.5 + 0 * s], 1), atol=TOL)
    for i in range(len(q)):
        np.testing.assert_allclose(o["fk"][i, 1, 3:].reshape(3, 3), rotm((0, 0, 1), s[i]), atol=TOL)


def test_fk_offcentre_hinge_slide_and_ref(exe, tmp_path):
    a = np.array([0.0, 0.9, -2.2])
    o = geom_fk(exe, tmp_path, "offc", S.offcentre_hinge(), 1, a[:, None])
    anchor, body, jp = np.array([0.4, 0, 0.6]), np.array([0.3, 0, 0.4]), np.array([0.1, 0, 0.2])
    for i, ai in enumerate(a):  # the body origin turns about the anchor
        np.testing.assert_allclose(o["fk"][i, 0, :3], anchor - rotm((0, 1, 0), ai) @ jp, atol=TOL)
    np.testing.assert_allclose(o["fk"][0, 0, :3], body, atol=TOL)
    o = geom_fk(exe, tmp_path, "slide", S.slider(0.1), 1, [[0.1], [0.6], [-0.4]])
    for i, v in enumerate((0.0, 0.5, -0.5)):  # metres along (0, 0.6, 0.8) from the drawn pose at q = ref
        np.testing.assert_allclose(o["fk"][i, 0, :3], np.array([0.1, 0.2, 0.3]) + v * np.array([0, 0.6, 0.8]), atol=TOL)
        np.testing.assert_allclose(o["fk"][i, 0, 3:], np.eye(3).reshape(-1), atol=TOL)
    o = geom_fk(exe, tmp_path, "ref", S.hinge_ref(0.7), 1, [[0.7], [0.7 + 0.5]])
    np.testing.assert_allclose(o["fk"][0, 0, :3], (0.1, 0.45, 0.3), atol=TOL)  # q = ref: the drawn pose
    np.testing.assert_allclose(o["fk"][1, 0, :3], np.array([0.1, 0.2, 0.3]) + rotm((1, 0, 0), 0.5) @ [0, 0.25, 0], atol=TOL)


def test_fk_rotated_parent_universal_free_base_and_frozen(exe, tmp_path):
    a = np.array([0.0, 0.8])
    o = geom_fk(exe, tmp_path, "rotp", S.rotated_parent(), 1, a[:, None])
    Rz = rotm((0, 0, 1), np.pi / 2)
    for i, ai in enumerate(a):
        want = np.array([0, 0, 0.5]) + Rz @ (np.array([0.2, 0, 0]) + rotm((1, 0, 0), ai) @ [0, 0.3, 0])
        np.testing.assert_allclose(o["fk"][i, 0, :3], want, atol=TOL)
        np.testing.assert_allclose(o["fk"][i, 0, 3:].reshape(3, 3), Rz @ rotm((1, 0, 0), ai), atol=TOL)
    q = np.array([[0.4, -0.9], [2.0, 1.3]])
    o = geom_fk(exe, tmp_path, "univ", S.universal(), 2, q)
    for i in range(2):  # the second hinge's axis has been turned by the first
        Rm = rotm((0, 0, 1), q[i, 0]) @ rotm((0, 1, 0), q[i, 1])
        np.testing.assert_allclose(o["fk"][i, 0, :3], np.array([0, 0, 0.5]) + Rm @ [0.3, 0, 0], atol=TOL)
    # D = 1 of the same body: the second hinge stays at qpos0
    o1 = geom_fk(exe, tmp_path, "univ1", S.universal(), 1, q[:, :1])
    for i in range(2):
        np.testing.assert_allclose(o1["fk"][i, 0, :3], np.array([0, 0, 0.5]) + rotm((0, 0, 1), q[i, 0]) @ [0.3, 0, 0], atol=TOL)
    # free base + hinge: D = 8 drives both, D = 7 freezes the hinge, D = 3 moves the base only
    c = np.sqrt(0.5)
    q8 = np.array([[0.1, 0.2, 0.3, c, 0, 0, c, 0.6]])
    Rb = rotm((0, 0, 1), np.pi / 2)
    for D, ang in ((8, 0.6), (7, 0.0)):
        o = geom_fk(exe, tmp_path, "fb%d" % D, S.free_base_hinge(), D, q8[:, :D])
        np.testing.assert_allclose(o["fk"][0, 0, :3], (0.1, 0.2, 0.3), atol=TOL)
        want = np.array([0.1, 0.2, 0.3]) + Rb @ (np.array([0, 0, 0.1]) + rotm((0, 1, 0), ang) @ [0.3, 0, 0])
        np.testing.assert_allclose(o["fk"][0, 1, :3], want, atol=TOL)
        assert o["info"]["n_driven_bodies"] == 2
    o = geom_fk(exe, tmp_path, "fb3", S.free_base_hinge(), 3, q8[:, :3])
    np.testing.assert_allclose(o["fk"][0, 1, :3], (0.1 + 0.3, 0.2, 0.3 + 0.1), atol=TOL)
    # D > nq is refused
    bad = H.chain(exe, world_xml(tmp_path, "fb9", S.free_base_hinge()), 9, np.zeros((1, 9)), tmp_path, tag="fb9")
    assert bad["rc"] == -1 and "nq" in bad["err"]


# ------------------------------------------------------------------ FK, random arms
@pytest.mark.parametrize("nj,seed,free_base", [(7, 3, False), (9, 4, False), (9, 5, True)])
def test_fk_random_arms(exe, tmp_path, nj, seed, free_base):
    """1000 poses against chain_ref: <= 1e-12 on positions and matrix entries.  The bar is derived:
    nine joints of a few ulp each on a metre-scale arm is about 1e-15; an error of rule is 1e-3 or more."""
    world = S.strip(S.random_arm(nj, seed, S.CAPSULE, free_base))
    m = R.flatten(world)
    D = m["nq"]
    q = S.arm_poses(D, 1000, seed + 100, spread=3.0, free_base=free_base)
    o = geom_fk(exe, tmp_path, "arm", world, D, q)
    _, _, gpos, gmat = R.fk(m, R.full_qpos(m, q))
    assert np.abs(o["fk"][:, :, :3] - gpos).max() <= 1e-12
    assert np.abs(o["fk"][:, :, 3:] - gmat).max() <= 1e-12
    assert np.ptp(gpos[:, -1], axis=0).min() > 0.5  # (the tool really moves)
    # frozen joints past D stay at qpos0
    D2 = D - 3
    o2 = geom_fk(exe, tmp_path, "arm_frozen", world, D2, q[:, :D2])
    _, _, gpos2, gmat2 = R.fk(m, R.full_qpos(m, q[:, :D2]))
    assert np.abs(o2["fk"][:, :, :3] - gpos2).max() <= 1e-12 and np.abs(o2["fk"][:, :, 3:] - gmat2).max() <= 1e-12


# ------------------------------------------------------------------ pair table
def test_pair_table(exe, tmp_path):
    world = S.capsule_arm_world(7, 11)
    world["excludes"] = [("link2", "link5")]
    # masks: the rail collides with nothing but the tool; a margin on the crate
    for g in world["geoms"]:
        if g["name"] == "rail":
            g["contype"], g["conaffinity"] = 2, 0
        if g["name"] == "crate":
            g["margin"] = 0.01

    def find(b):  # the tool answers the rail's contype
        for g in b.get("geoms", ()):
            if g["name"] == "tool":
                g["conaffinity"] = 3
        for c in b.get("children", ()):
            find(c)
    find(world["bodies"][0])
    m = R.flatten(world)
    D = 7
    o = H.chain(exe, world_xml(tmp_path, "pairs", world), D, np.zeros((1, D)), tmp_path)
    assert o["rc"] == 0, o["err"]
    mv, st = R.pairs(m, D)
    assert [(p[0], p[1]) for p in o["pairs"]] == [(p[0], p[1]) for p in mv]
    assert [p[4] for p in o["pairs"]] == [p[2] for p in mv]
    names = [g["name"] for g in m["geoms"]]
    got = {(names[p[0]], names[p[1]]) for p in o["pairs"]}
    assert ("lg0", "lg1") not in got and ("lg3", "lg4") not in got           # adjacent links skipped
    assert ("floor", "lg3") in got and ("crate", "lg0") in got                # link-world kept
    assert ("lg0", "lg2") in got and ("lg1", "tool") in got                   # self-collision present
    assert ("lg2", "lg5") not in got and ("lg2", "lg4") in got                # <exclude>
    assert ("rail", "tool") in got and ("rail", "lg3") not in got             # masks
    assert dict(((names[p[0]], names[p[1]]), p[4]) for p in o["pairs"])[("crate", "lg1")] == 0.01
    for g1, g2, m1, m2, _ in o["pairs"]:
        assert (m1, m2) == (int(m["geoms"][g1]["body"] != 0), int(m["geoms"][g2]["body"] != 0))
    assert o["info"]["n_pairs"] == len(mv) and o["info"]["n_static_pairs"] == len(st)
    # D = 3: links 3.. are frozen but ride driven ancestors; nothing of the arm is static
    o3 = H.chain(exe, world_xml(tmp_path, "pairs", world), 3, np.zeros((1, 3)), tmp_path)
    assert [(p[0], p[1]) for p in o3["pairs"]] == [(p[0], p[1]) for p in R.pairs(m, 3)[0]]
    assert o3["info"]["n_driven_bodies"] == 7


def test_capsule_cylinder_pair_refused(exe, tmp_path):
    world = S.capsule_arm_world(3, 2)
    world["geoms"].append(dict(name="drum", type=S.CYLINDER, size=(0.1, 0.2, 0), pos=(1, 1, 0.2)))
    o = H.chain(exe, world_xml(tmp_path, "capcyl", world), 3, np.zeros((1, 3)), tmp_path)
    assert o["rc"] == -5 and "drum" in o["err"] and "unsupported collision pair" in o["err"]


# ------------------------------------------------------------------ contact decisions
MAX_NEAR_PER_1000 = 2
N_POSES = 2000

# (name, joints, arm seed, free base, pose seed, spread): the seeds are the first of 1, 2, .. at which
# the reference alone leaves out at most 2 poses per 1000 and has between 10 % and 90 % touching
CAPSULE_SCENES = [("arm7", 7, 11, False, 1, 2.0), ("arm9_free", 9, 12, True, 1, 2.0)]


@pytest.fixture(scope="module")
def capsule_cases():
    made = {}

    def get(name):
        if name not in made:
            _, nj, aseed, fb, pseed, spread = next(s for s in CAPSULE_SCENES if s[0] == name)
            world = S.capsule_arm_world(nj, aseed, fb)
            m = R.flatten(world)
            D = m["nq"]
            q = S.arm_poses(D, N_POSES, pseed, spread, fb)
            hit, near, per_pair = R.contacts(m, D, q)
            for a in (q, hit, near, per_pair):
                a.setflags(write=False)
            made[name] = dict(world=world, m=m, D=D, q=q, hit=hit, near=near, per_pair=per_pair)
        return made[name]

    return get


def assert_reference_informative(c):
    frac = c["hit"][~c["near"]].mean()
    print("reference: %d near poses of %d, %.1f %% touching" % (c["near"].sum(), len(c["near"]), 100 * frac))
    assert c["near"].sum() <= MAX_NEAR_PER_1000 * len(c["near"]) // 1000
    assert 0.10 <= frac <= 0.90


@pytest.mark.parametrize("name", [s[0] for s in CAPSULE_SCENES])
def test_contacts_capsule_arm(exe, tmp_path, capsule_cases, name):
    """scene 1: a capsule-link arm with a sphere tool over a floor, beside a box and capsule posts"""
    c = capsule_cases(name)
    assert_reference_informative(c)
    types = {tuple(sorted((c["m"]["geoms"][a]["type"], c["m"]["geoms"][b]["type"]))) for a, b, _ in R.pairs(c["m"], c["D"])[0]}
    assert {(0, 2), (0, 3), (2, 3), (2, 6), (3, 3), (3, 6)} <= types
    touching = {t for t in types if any(c["per_pair"][:, k].any() for k, (a, b, _) in enumerate(R.pairs(c["m"], c["D"])[0])
                                        if tuple(sorted((c["m"]["geoms"][a]["type"], c["m"]["geoms"][b]["type"]))) == t)}
    assert len(touching) >= 4, touching
    o = H.chain(exe, world_xml(tmp_path, name, c["world"]), c["D"], c["q"], tmp_path)
    assert o["rc"] == 0, o["err"]
    keep = ~c["near"]
    np.testing.assert_array_equal(o["hit"][keep].astype(bool), c["hit"][keep])


def test_contacts_box_cylinder_arm_frozen_twin(exe, tmp_path):
    """scene 2: box and cylinder links; the reference's decisions come from the frozen twin"""
    world = S.box_cyl_arm_world(5, 5)
    m = R.flatten(world)
    D = m["nq"]
    q = S.arm_poses(D, N_POSES, 1, 2.0)
    o = H.chain(exe, world_xml(tmp_path, "boxcyl", world), D, q, tmp_path)
    assert o["rc"] == 0, o["err"]
    t = H.twin(exe, world_xml(tmp_path, "boxcyl_twin", R.twin_world(world, m)), R.twin_qpos(m, q), tmp_path)
    assert t["rc"] == 0, t["err"]
    assert t["pairs"] == [(p[0], p[1]) for p in o["pairs"]]
    types = {tuple(sorted((m["geoms"][a]["type"], m["geoms"][b]["type"]))) for a, b in t["pairs"]}
    assert {(0, 5), (0, 6), (2, 5), (2, 6), (5, 5), (5, 6), (6, 6)} <= types
    want = (t["contact"] > 0).any(1)
    frac = want.mean()
    print("frozen twin: %.1f %% touching" % (100 * frac))
    assert 0.10 <= frac <= 0.90
    # (the twin has no distances: no pose is left out)
    np.testing.assert_array_equal(o["hit"].astype(bool), want)


def crafted_world():
    """a tool sphere on a yaw hinge and two slides: `drop` lowers it to the floor, `reach` pushes
    it (after a quarter turn of the yaw) against a vertical capsule post"""
    r = 0.04
    ram = dict(name="ram", pos=(0.3, 0, 0), joints=[dict(type="slide", axis=(0, 0, -1), name="drop"),
                                                     dict(type="slide", axis=(1, 0, 0), name="reach")],
               geoms=[dict(name="tool", type=S.SPHERE, size=(r, 0, 0))])
    col = dict(name="col", pos=(0, 0, 0.5), joints=[dict(type="hinge", axis=(0, 0, 1), name="yaw")],
               geoms=[dict(name="colg", type=S.CAPSULE, size=(0.02, 0.05, 0), pos=(0, 0, 0.3))], children=[ram])
    post = dict(name="post", type=S.CAPSULE, size=(0.05, 0.3, 0), pos=(0, 0.6, 0.5))
    return dict(geoms=[dict(name="floor", type=S.PLANE, size=(0, 0, 1)), post], bodies=[col]), r


def crafted_poses(r):
    """(yaw, drop, reach) with the tool eps from touching: the floor (rows 0-3), the post (rows 4-7);
    eps = +1e-9, -1e-9, +1e-6, -1e-6"""
    eps = np.array([1e-9, -1e-9, 1e-6, -1e-6])
    z = np.zeros(4)
    floor = np.stack([z, 0.5 - r - eps, z], 1)                       # centre height r + eps
    post = np.stack([z + np.pi / 2, z, 0.6 - 0.3 - r - 0.05 - eps], 1)  # centre r + 0.05 + eps from the post's axis
    return np.concatenate([floor, post])


def test_crafted_thresholds(exe, tmp_path):
    """a tool sphere at +-1e-9 and +-1e-6 around touching the floor and the post, reached through
    the joints, decided as capsule_ref decides (1e-9 m is a million ulp at this scale)"""
    world, r = crafted_world()
    m = R.flatten(world)
    q = crafted_poses(r)
    hit, near, per_pair = R.contacts(m, 3, q)
    assert hit.tolist() == [False, True, False, True] * 2
    assert not near[[2, 3, 6, 7]].any()
    names = [g["name"] for g in m["geoms"]]
    cols = [(names[a], names[b]) for a, b, _ in R.pairs(m, 3)[0]]
    assert per_pair[1, cols.index(("floor", "tool"))] and per_pair[5, cols.index(("post", "tool"))]
    assert per_pair.sum() == 4  # (nothing else touches)
    o = H.chain(exe, world_xml(tmp_path, "crafted", world), 3, q, tmp_path)
    assert o["rc"] == 0, o["err"]
    np.testing.assert_array_equal(o["hit"].astype(bool), hit)


# ------------------------------------------------------------------ sanitizers
def test_host_program_under_sanitizers(exe, exe_san, tmp_path, capsule_cases):
    """the same program with -fsanitize=address,undefined, run as a program: clean, same bytes"""
    xml = H.write_xml(tmp_path, "loader", LOADER_XML)
    a, b = H.load(exe_san, xml), H.load(exe, xml)
    assert a["lines"] == b["lines"]
    c = capsule_cases("arm9_free")
    x = world_xml(tmp_path, "arm9", c["world"])
    s = H.chain(exe_san, x, c["D"], c["q"][:300], tmp_path, tag="san")
    p = H.chain(exe, x, c["D"], c["q"][:300], tmp_path, tag="plain")
    for o in (a, s):
        assert "runtime error" not in o["stderr"] and "AddressSanitizer" not in o["stderr"], o["stderr"][-2000:]
    assert s["fk"].tobytes() == p["fk"].tobytes() and s["hit"].tobytes() == p["hit"].tobytes()
    world = S.box_cyl_arm_world(5, 5)
    m = R.flatten(world)
    q = S.arm_poses(m["nq"], 50, 1, 2.0)
    t = H.twin(exe_san, world_xml(tmp_path, "twin", R.twin_world(world, m)), R.twin_qpos(m, q), tmp_path)
    assert t["rc"] == 0 and "runtime error" not in t["stderr"] and "AddressSanitizer" not in t["stderr"]
