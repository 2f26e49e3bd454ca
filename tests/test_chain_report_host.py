"""The contact report for arms on the host, without a GPU: tests/chain_report/check_chain_report.cpp
runs sspc::chain_build and the per-pose routines sspc::chain_pair_report / chain_first_pair
(sspp_chain_report.h: the code the report's kernels loop over).  Capsule arms are checked count for
count against tests/chain_report_ref.py (numpy, written from the rule, no product code); box and
cylinder links against the frozen twin's per-pair counts (every link a free body at the reference's
pose, the scene builder's env-env path).  A second build of the same program runs under
AddressSanitizer / UBSan (a stand-alone program).
"""
import numpy as np
import pytest

from tests import chain_host as H
from tests import chain_ref as R
from tests import chain_report_host as RH
from tests import chain_report_ref as RR
from tests import chain_scenes as S

N_POSES = 2000
# (joints, arm seed, free base): tests/test_gpu_chain.py's arm3, arm7, arm9 and base2
CAPSULE_ARMS = [(3, 21, False), (7, 11, False), (9, 23, False), (2, 24, True)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chain_report") / "check_chain_report")
    r = RH.build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def exe_chain(tmp_path_factory):
    """tests/chain/check_chain.cpp: chain_contact's decision, for the invariants"""
    out = str(tmp_path_factory.mktemp("chain_report_old") / "check_chain")
    r = H.build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    """the program under ASan / UBSan; skipped only when a one-line program cannot be built and run
    with the same flags (no sanitizer runtime) — check_chain_report.cpp itself must then build"""
    d = tmp_path_factory.mktemp("chain_report_san")
    why = H.sanitizer_probe(d)
    if why:
        pytest.skip("no sanitizer runtime on this machine: " + why)
    out = str(d / "check_chain_report_san")
    r = RH.build(out, H.SAN_FLAGS)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def world_xml(tmp, name, world):
    return H.write_xml(tmp, name, S.mjcf(world))


def check_invariants(o, old):
    """on every set: contact.any(1) is chain_contact's hit, first is the lowest nonzero column, the
    report without deep has the same contact bytes, no entry is left unwritten, the static pairs'
    contacts sum to static_contacts"""
    assert old["rc"] == 0, old["err"]
    assert o["pairs"] == old["pairs"] and o["info"] == old["info"]
    assert not (o["contact"] == 0xee).any() and not (o["deep"] == 0xee).any()
    np.testing.assert_array_equal((o["contact"] > 0).any(1), old["hit"].astype(bool))
    np.testing.assert_array_equal(o["first"], RH.first_of(o["contact"]))
    assert o["contact_only"].tobytes() == o["contact"].tobytes()
    assert len(o["statics"]) == o["info"]["n_static_pairs"]
    assert sum(s[3] for s in o["statics"]) == o["info"]["static_contacts"]


@pytest.mark.parametrize("nj,seed,fb", CAPSULE_ARMS)
def test_capsule_arm_counts_equal_reference(exe, exe_chain, tmp_path, nj, seed, fb):
    """2000 poses, every pair, count for count; no pose is left out: the reference's distances stay
    1e-9 clear of every threshold (the closest of the four sets is 9.4e-7)"""
    world = S.capsule_arm_world(nj, seed, fb)
    m = R.flatten(world)
    D = m["nq"]
    q = S.arm_poses(D, N_POSES, seed + 7, 2.0, fb)
    contact, deep, gap = RR.report(m, D, q)
    print("reference: gap %.3g, %.1f %% of poses touch, %d of %d pairs hit, %d entries == 2, %d shallow, %.1f %% multi"
          % (gap, 100 * (contact > 0).any(1).mean(), (contact > 0).any(0).sum(), contact.shape[1], (contact == 2).sum(),
             ((contact > 0) & (deep == 0)).sum(), 100 * ((contact > 0).sum(1) >= 2).mean()))
    # floors, from the reference alone
    assert gap > 1e-9
    assert ((contact > 0) & (deep == 0)).any()
    assert ((contact > 0).sum(1) >= 2).any()
    if nj != 3:  # (the 3-joint set never reaches two contacts on one pair)
        assert (contact == 2).any()
    xml = world_xml(tmp_path, "arm", world)
    o = RH.chain(exe, xml, D, q, tmp_path)
    assert o["rc"] == 0, o["err"]
    assert [(p[0], p[1]) for p in o["pairs"]] == [(p[0], p[1]) for p in R.pairs(m, D)[0]]
    np.testing.assert_array_equal(o["contact"], contact)
    np.testing.assert_array_equal(o["deep"], deep)
    check_invariants(o, H.chain(exe_chain, xml, D, q, tmp_path))


def test_arm7_reference_is_informative():
    """the 7-joint set, from the reference alone: most poses touch, most pairs are hit, two-contact
    entries, shallow contacts and multi-pair poses are all common"""
    m = R.flatten(S.capsule_arm_world(7, 11))
    contact, deep, _ = RR.report(m, 7, S.arm_poses(7, N_POSES, 11 + 7, 2.0))
    assert contact.shape[1] == 52
    assert (contact > 0).any(1).mean() > 0.5 and (contact > 0).any(0).sum() >= 26
    assert (contact == 2).sum() >= 100 and ((contact > 0) & (deep == 0)).sum() >= 10
    assert ((contact > 0).sum(1) >= 2).mean() > 0.25


# A crafted pose of box_cyl_arm_world(5, 5) is not needed: the twin shows box-box entries with
# deep > contact among the 2000 poses (asserted below before the comparison).
def test_box_cylinder_arm_counts_equal_frozen_twin(exe, exe_chain, tmp_path):
    """box and cylinder links: per-pair counts against the frozen twin's, pairs matched by geom index"""
    world = S.box_cyl_arm_world(5, 5)
    m = R.flatten(world)
    D = m["nq"]
    q = S.arm_poses(D, N_POSES, 5 + 7, 2.0)
    xml = world_xml(tmp_path, "boxcyl", world)
    o = RH.chain(exe, xml, D, q, tmp_path)
    assert o["rc"] == 0, o["err"]
    t = RH.twin(exe, world_xml(tmp_path, "boxcyl_twin", R.twin_world(world, m)), R.twin_qpos(m, q), tmp_path)
    assert t["rc"] == 0, t["err"]
    cols = {p: k for k, p in enumerate(t["pairs"])}
    idx = [cols[(p[0], p[1])] for p in o["pairs"]]  # (every chain pair is a twin pair)
    want_c, want_d = t["contact"][:, idx], t["deep"][:, idx]
    types = [tuple(sorted((m["geoms"][p[0]]["type"], m["geoms"][p[1]]["type"]))) for p in o["pairs"]]
    assert {(0, 5), (0, 6), (2, 5), (2, 6), (5, 5), (5, 6), (6, 6)} <= set(types)
    bb = np.array([ty == (6, 6) for ty in types])
    n_bb = int((want_d[:, bb] > want_c[:, bb]).sum())
    print("frozen twin: %.1f %% touching, %d box-box entries with deep > contact" % (100 * (want_c > 0).any(1).mean(), n_bb))
    assert n_bb > 0
    assert 0.10 <= (want_c > 0).any(1).mean() <= 0.90
    assert ((want_c > 0) & (want_d == 0)).any() and ((want_c > 0).sum(1) >= 2).any()
    np.testing.assert_array_equal(o["contact"], want_c)
    np.testing.assert_array_equal(o["deep"], want_d)
    check_invariants(o, H.chain(exe_chain, xml, D, q, tmp_path))


def static_block_world(z):
    """capsule_arm_world(3, 21) and a block on a body of its own whose hinge (qpos address 3) lies
    past the 3 driven values: the body is static, and its pairs with the world's geoms are
    static-static.  z = 0.1 rests the block (half height 0.1) on the floor."""
    world = S.capsule_arm_world(3, 21)
    world["bodies"].append(dict(name="gate", pos=(3, 3, z), joints=[dict(type="hinge", axis=(0, 0, 1))],
                                geoms=[dict(name="block", type=S.BOX, size=(0.1, 0.1, 0.1))]))
    return world


def test_static_pairs(exe, exe_chain, tmp_path):
    """the static pairs with their counts: a world with a static block resting on the floor (the
    plane-box pair's contacts, nonzero) and the same world with the block lifted (zero)"""
    for name, z, touching in (("rest", 0.1, True), ("lift", 0.15, False)):
        world = static_block_world(z)
        m = R.flatten(world)
        xml = world_xml(tmp_path, name, world)
        q = S.arm_poses(3, 10, 1, 2.0)
        o = RH.chain(exe, xml, 3, q, tmp_path, tag=name)
        assert o["rc"] == 0, o["err"]
        assert [(s[0], s[1], s[2]) for s in o["statics"]] == [tuple(p) for p in R.pairs(m, 3)[1]]
        names = [g["name"] for g in m["geoms"]]
        by = {(names[s[0]], names[s[1]]): s for s in o["statics"]}
        assert len(by) == 4 and (by[("floor", "block")][3] > 0) == touching
        assert all(s[3] == 0 and s[4] == 0 for k, s in by.items() if k != ("floor", "block"))
        assert (o["info"]["static_contacts"] > 0) == touching
        check_invariants(o, H.chain(exe_chain, xml, 3, q, tmp_path, tag=name + "_old"))


def test_empty_and_single_pair_tables(exe, exe_chain, tmp_path):
    """P = 0 (every geom contype = conaffinity = 0) and P = 1 (one link, one ball)"""
    world = S.capsule_arm_world(3, 21)

    def off(b):
        for g in b.get("geoms", ()):
            g["contype"], g["conaffinity"] = 0, 0
        for c in b.get("children", ()):
            off(c)
    for g in world["geoms"]:
        g["contype"], g["conaffinity"] = 0, 0
    off(world["bodies"][0])
    q = S.arm_poses(3, 5, 1, 2.0)
    o = RH.chain(exe, world_xml(tmp_path, "empty", world), 3, q, tmp_path, tag="empty")
    assert o["rc"] == 0 and o["info"]["n_pairs"] == 0 and o["contact"].shape == (5, 0) and (o["first"] == -1).all()
    one = dict(geoms=[dict(name="ball", type=S.SPHERE, size=(0.1, 0, 0), pos=(0.2, 0, 1.0))],
               bodies=[dict(name="s", pos=(0, 0, 1.0), joints=[dict(type="hinge", axis=(0, 1, 0))],
                            geoms=[dict(name="sg", type=S.SPHERE, size=(0.05, 0, 0), pos=(0, 0, 0.2))])])
    q = np.linspace(-2, 2, 41)[:, None]
    xml = world_xml(tmp_path, "one", one)
    o = RH.chain(exe, xml, 1, q, tmp_path, tag="one")
    assert o["rc"] == 0 and o["info"]["n_pairs"] == 1
    # the link's sphere swings through the ball about q = pi / 2: |(0.2 sin q - 0.2, 0.2 cos q)| <= 0.15
    want = np.hypot(0.2 * np.sin(q[:, 0]) - 0.2, 0.2 * np.cos(q[:, 0])) <= 0.15
    np.testing.assert_array_equal(o["contact"][:, 0] > 0, want)
    assert want.any() and not want.all()
    check_invariants(o, H.chain(exe_chain, xml, 1, q, tmp_path, tag="one_old"))


def test_host_program_under_sanitizers(exe, exe_san, tmp_path):
    """the same program with -fsanitize=address,undefined, run as a program: clean, same bytes; one
    capsule case and one twin case"""
    world = S.capsule_arm_world(9, 23)
    m = R.flatten(world)
    q = S.arm_poses(m["nq"], 300, 30, 2.0)
    xml = world_xml(tmp_path, "arm9", world)
    s = RH.chain(exe_san, xml, m["nq"], q, tmp_path, tag="san")
    p = RH.chain(exe, xml, m["nq"], q, tmp_path, tag="plain")
    assert "runtime error" not in s["stderr"] and "AddressSanitizer" not in s["stderr"], s["stderr"][-2000:]
    for k in ("contact", "deep", "first", "contact_only"):
        assert s[k].tobytes() == p[k].tobytes()
    assert s["statics"] == p["statics"]
    world = S.box_cyl_arm_world(5, 5)
    m = R.flatten(world)
    q = S.arm_poses(m["nq"], 50, 1, 2.0)
    txml = world_xml(tmp_path, "twin", R.twin_world(world, m))
    t = RH.twin(exe_san, txml, R.twin_qpos(m, q), tmp_path, tag="tsan")
    t0 = RH.twin(exe, txml, R.twin_qpos(m, q), tmp_path, tag="tplain")
    assert t["rc"] == 0 and "runtime error" not in t["stderr"] and "AddressSanitizer" not in t["stderr"]
    assert t["contact"].tobytes() == t0["contact"].tobytes() and t["deep"].tobytes() == t0["deep"].tobytes()
