"""The envelope scenes (tests/envelope_scenes.py) checked from the reference alone, before any of
their poses reaches a GPU: every pose with |off| >= boundary_poses.FLOOR is in contact exactly when
its offset is negative — at 16 m magnitudes too, FLOORS stays empty — both outcomes occur for every
pair type, case and quaternion family of every scene, the scenes sit where in the envelope their
names say (root coordinates, partner positions, extents, the scan f32_eps's rule gives them), and
the offsets straddle each table's own eps.  The host build of the device's FP64 decision
(sspd::pair_near, then sspd::collide) must agree with the reference on every pose."""
import numpy as np
import pytest

from tests import boundary_poses as BP
from tests import envelope_scenes as E
from tests import synth_scenes as Y
from tests.test_boundary_poses import hexrow, host_check  # noqa: F401  (host_check: a fixture)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("envelope_scenes"))


@pytest.mark.parametrize("margin", E.MARGINS)
@pytest.mark.parametrize("name", E.SCENES)
def test_decision_follows_the_offset_sign(root, name, margin):
    ref, cases, P, eps = E.envelope_set(root, name, margin)
    assert BP.FLOOR == 1e-9 and BP.FLOORS == {}
    assert len(cases) % len(E.QUATS) == 0 and 200 <= len(P["q"]) <= 900
    assert P["q"].shape[1] == E.DOF[name]
    hit = np.array([ref.contacts(q)[0] > 0 for q in P["q"]])
    assert np.array_equal(hit, P["off"] < 0)   # every |off| here is >= FLOOR
    assert np.abs(P["off"]).min() == 1e-9
    seen = {}
    for i, k in enumerate(P["case"]):
        c = cases[k]
        for key in (("pair", c["pair"]), ("case", c["pair"], c["feature"]), ("family", c["family"])):
            seen.setdefault(key, set()).add(bool(hit[i]))
    assert all(v == {True, False} for v in seen.values())
    assert {k[1] for k in seen if k[0] == "family"} == set("abcde")
    # 1 m on along d (the approach and mirrored candidates' other rows) nothing touches
    back = P["back"] if "back" in P else np.concatenate([P["q"][:, :3] + P["d"], P["q"][:, 3:]], axis=1)
    assert not any(ref.contacts(q)[0] for q in back[::3])


@pytest.mark.parametrize("name", E.SCENES)
def test_offsets_straddle_the_tables_eps(root, name):
    for margin in E.MARGINS:
        ref, cases, P, eps = E.envelope_set(root, name, margin)
        S = E.table_extent(ref.ref, E.DOF[name])
        assert eps == 2e-4 * S and S >= 1.0
        mags = np.unique(np.abs(P["off"]))
        assert len(mags) == 9 and (mags < 0.3 * eps).sum() >= 4 and ((mags > 0.3 * eps) & (mags < eps)).sum() == 2
        assert (mags > eps).sum() == 3 and mags.max() == 4.0 * eps


def test_scenes_sit_where_their_names_say(root):
    ext = {}
    for name in E.SCENES:
        for margin in E.MARGINS:
            ref, cases, P, eps = E.envelope_set(root, name, margin)
            r = ref.ref
            ext[name, margin] = S = E.table_extent(r, E.DOF[name])
            assert Y.expected_scan(r, E.DOF[name]) == E.SCAN[name], (name, margin)
            assert 2 <= len(Y.moving_pairs(r, E.DOF[name])) <= 8
            if name in E.ROOT_RANGE:
                lo, hi = E.ROOT_RANGE[name]
                a = np.abs(P["q"][:, :3])
                assert lo <= a.min() and a.max() <= hi, (name, a.min(), a.max())
            elif E.SCAN[name] != "fp64":
                assert np.abs(P["q"][:, :3]).max() <= 7.99   # every other filtered scene's poses lie inside the cube
            statics = np.array([r["geom_pos"][g] for g in range(len(r["geom_type"])) if r["geom_body"][g] == 0])
            assert (np.abs(statics).max() > 16.0) == (name == "far_partner_out")
    for margin in E.MARGINS:
        assert 7.6 < ext["far_partner", margin] <= 8.0 and 7.6 < ext["far_partner_out", margin] <= 8.0
        assert abs(ext["large2", margin] - 2.0) < 0.05 and abs(ext["large4", margin] - 4.0) < 0.05
        assert abs(ext["large7", margin] - 7.5) < 0.05 and 8.0 < ext["large_over", margin] < 8.1
        assert 1.6 < ext["offset_one", margin] < 1.8 and ext["offset_two", margin] == ext["offset_one", margin]
        assert ext["far_in", margin] == ext["far_out", margin] == ext["movers", margin] == 1.0
    # far_partner's touching root: x = 7.8 .. 7.95 m from a partner centred 15.5 m out
    _, cases, P, _ = E.envelope_set(root, "far_partner", 0.0)
    wall = np.array([cases[k]["target"] == "wall" for k in P["case"]])
    assert 7.8 <= P["q"][wall, 0].min() and P["q"][wall, 0].max() <= 7.95
    # the offset scenes' geoms hang 1.5 and 1.3 m off the root with rotations of their own
    assert abs(np.linalg.norm(E.GEOM_A["pos"]) - 1.5) < 0.01 and abs(np.linalg.norm(E.GEOM_B["pos"]) - 1.3) < 0.02


@pytest.mark.parametrize("name", E.SCENES)
def test_host_fp64_decision_on_envelope_poses(root, host_check, name):  # noqa: F811
    """The target pair of every pose through the host build of pair_near and collide: a contact
    exactly where the offset is negative.  pair_near's box cull once rejected poses of offset_two
    (margin 1e-2, the second geom off an edge of the tilted box) that the SAT, and the reference,
    report in contact."""
    for margin in E.MARGINS:
        ref, cases, P, _ = E.envelope_set(root, name, margin)
        ty, size, mg = ref.ref["geom_type"], np.asarray(ref.ref["geom_size"], float), ref.ref["geom_margin"]
        rows = []
        for q, k in zip(P["q"], P["case"]):
            c = cases[k]
            xp, xm = ref.full.fk(q)
            gm, gt = ref.geom(c.get("geom", "m_geom")), ref.geom(c["target"])
            a, b = (gm, gt) if (ty[gm], gm) < (ty[gt], gt) else (gt, gm)
            rows.append(hexrow([ty[a], ty[b], max(mg[gm], mg[gt])], xp[a], xm[a], size[a], xp[b], xm[b], size[b],
                               [1 if a == gm else 2]))
        nc, nd, cb2, outl, up, near = host_check(rows).T
        np.testing.assert_array_equal((near == 1) & (nc > 0), P["off"] < 0, err_msg="%s margin %g" % (name, margin))
