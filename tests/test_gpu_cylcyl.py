"""GPU parity on cylinder-cylinder scenes: k_sspp_c2f / k_sspp_census, k_tsp and its forms,
k_tsp_group and the drop-in modules against the composed reference of tests/cylcyl_scenes.py (the
CPU oracle on a copy of the scene with the cylinder-cylinder pairs filtered out by their bits +
tests/cylcyl_ref.py on those pairs; the oracle knows no such pair).

Bars: test_gpu_capsule.py's — sampled control points bit-equal to the oracle's, flags equal, arcs
within COST_TOL, best record equal; the synthetic scenes' 1e-9 for TaskSpacePlanner costs.  A
candidate with a cylinder-cylinder waypoint within the reference's band (cylcyl_ref.BAND) of a
threshold is left out: at most 8 of 2048, chosen from the reference alone.  The estimate behind
the cap: waypoints lie >~ 5 mm apart along a path, so a threshold crossing puts a waypoint inside
a band of 2 x 5e-9 with probability ~2e-6, far under one candidate per 2048.
Every case asserts, from the reference alone, that it is not vacuous.  Before cylinder-cylinder
pairs were supported every test here failed at Scene(...) with (-5).
"""
import os

import numpy as np
import pytest

from oracle import mjcf_ref
from oracle import oracle as O
from tests import cylcyl_ref as R
from tests import cylcyl_scenes as CC
from tests import synth_scenes as Y
from tests.conftest import arc_err
from tests.test_collision_exact import _mat_to_quat
from tests.test_gpu_parity import COST_TOL, SHAPES, _np, linear_init, run_sspp

pytestmark = pytest.mark.gpu

LAUNCH = [(0, 0), (128, 4), (64, 3), (256, 64)]
assert set(LAUNCH) <= set(SHAPES)
B, W, N_CTRL, D = 2048, 64, 10, 7
SEED = 7
MIN_EACH, NEAR_CAP = 16, 8
SSPP_SCENES = {"i": CC.sspp_cyl_mover, "ii": CC.sspp_two_geom_mover, "iii": CC.sspp_ten_pairs,
               "iv": CC.sspp_static_contact}


class Bundle:
    def __init__(self, root, name, scene, mode, arg, count_static=True):
        import sspp_amd as S
        st, bodies = scene() if callable(scene) else scene
        self.path = os.path.join(root, name + ".xml")
        with open(self.path, "w") as f:
            f.write(Y.mjcf(st, bodies))
        self.model = S.Model(self.path)
        self.ref = mjcf_ref.load(self.path)
        Y.assert_loaders_agree(self.model.arrays(), self.ref)
        if isinstance(arg, str):
            arg = self.ref["body_names"].index(arg)
        self.mode, self.arg = mode, arg
        self.scene = S.Scene(self.model, mode, arg, count_static=count_static)
        self.memo = {}


@pytest.fixture(scope="module")
def bundles(cuda, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("cylcyl_scenes"))
    made = {}

    def get(name, scene, mode=0, arg=D, count_static=True):
        key = (name, mode, arg, count_static)
        if key not in made:
            made[key] = Bundle(root, "%s_%d" % (name, len(made)), scene, mode, arg, count_static)
        return made[key]

    return get


# ------------------------------------------------------------------ SamplingPathPlanner
def sspp_ref(b):
    """The scene's candidates and their composed reference, once per scene."""
    if "sspp" not in b.memo:
        knots, ctrl0 = linear_init(CC.START, CC.END, N_CTRL)
        ctrl = O.sample_sspp(ctrl0, 3, CC.SIGMA, CC.LIMITS, SEED, 0, B)
        r = CC.sspp_reference(b.ref, knots, ctrl, W, D)
        for a in [ctrl] + [v for v in r.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        b.memo["sspp"] = (knots, ctrl0, ctrl, r)
    return b.memo["sspp"]


def assert_not_vacuous(r):
    nf = int(r["feas"].sum())
    assert MIN_EACH <= nf <= B - MIN_EACH, nf
    assert int(r["near"].sum()) <= NEAR_CAP
    # candidates a cylinder-cylinder pair alone decides
    assert int((r["feas_nocc"].astype(bool) & r["hit"].any(1)).sum()) >= 1


def sspp_case(b, nt, g1, order=None):
    import sspp_amd as S
    knots, ctrl0, ctrl, r = sspp_ref(b)
    job = S.SsppJob(b.scene, knots, 3, ctrl0, CC.SIGMA, CC.LIMITS, W, seed=SEED, max_batch=B)
    job.set_shape(nt, g1)
    if order is not None:
        job.set_option(S.OPT_ORDER, order)
    got = run_sspp(job, B)
    assert np.array_equal(got["ctrl"], ctrl)  # so the reference scored what the GPU scored
    keep = ~r["near"]
    np.testing.assert_array_equal(got["feasible"][keep], r["feas"][keep])
    assert arc_err(got["arc"][keep], r["arc"][keep]) <= COST_TOL
    if keep.all():
        idx_o, best_o = O.argmin(r["arc"], r["feas"])
        cost, idx, cnt = got["best"]
        assert cnt == int(r["feas"].sum()) and idx == idx_o
        assert abs(cost - best_o) <= COST_TOL
    assert job.get_option(S._lib.OPT_CYLCYL) == 1 and job.config()["cylinder_cylinder"]
    assert not job.config()["capsule"] and not job.config()["split"]
    return job, got, r


@pytest.mark.parametrize("nt,g1", LAUNCH)
@pytest.mark.parametrize("case", ["i", "ii", "iii"])
def test_sspp_cylinder_scenes_match_reference(bundles, case, nt, g1):
    """(i) a cylinder mover against a vertical and a tilted static cylinder, the tilted plane and a
    box; (ii) a box + cylinder mover (ONEGEOM false) in a table with box-box pairs: the
    FP32-filtered scan settles those and leaves the cylinder pairs to FP64; (iii) 10 pairs: the
    survivors' hull masks run."""
    b = bundles(case, SSPP_SCENES[case])
    job, got, r = sspp_case(b, nt, g1)
    assert_not_vacuous(r)
    npairs = len(Y.moving_pairs(b.ref, D))
    assert job.config()["sampled_pairs"] == b.scene.info()["n_pairs"] == npairs
    assert npairs == {"i": 4, "ii": 7, "iii": 10}[case]
    assert job.config()["cylinder_box"]
    if case != "i":
        assert job.config()["scan"] == "fp32-filtered"
        types = {tuple(sorted((b.ref["geom_type"][a], b.ref["geom_type"][c]))) for a, c in Y.moving_pairs(b.ref, D)}
        assert {(6, 6), (0, 6), (5, 5), (5, 6)} <= types


@pytest.mark.parametrize("order", [0, 1, 2])
def test_sspp_cylinder_scan_orders(bundles, order):
    """Every pair / waypoint scan order (the census kernel runs for order 2) gives the same results."""
    sspp_case(bundles("iii", SSPP_SCENES["iii"]), 0, 0, order=order)


def test_sspp_static_cylinder_contact(bundles):
    """(iv) two cylinders 5 mm into each other, both static for the planner: static_contacts is the
    reference's 1 (and the TaskSpacePlanner scene's static_cost its term), count_static makes
    every candidate infeasible, and without it the scene scores like (i)."""
    import sspp_amd as S
    b = bundles("iv", SSPP_SCENES["iv"])
    occ = O.Scene(CC.oracle_copy(b.ref), 0, D)
    mover = b.ref["body_names"].index("mover")
    want_n, want_cost = CC.static_cc_contacts(b.ref, occ, {mover})
    assert want_n == 1 and want_cost < -1.0
    assert b.scene.info()["static_contacts"] == 1
    tsp = bundles("iv", SSPP_SCENES["iv"], 1, "mover")
    assert tsp.scene.info()["static_contacts"] == 1 and abs(tsp.scene.info()["static_cost"] - want_cost) <= 1e-12
    knots, ctrl0, ctrl, r = sspp_ref(b)
    job = S.SsppJob(b.scene, knots, 3, ctrl0, CC.SIGMA, CC.LIMITS, W, seed=SEED, max_batch=B)
    got = run_sspp(job, B)
    assert np.array_equal(got["ctrl"], ctrl)
    assert not got["feasible"].any() and np.isinf(got["arc"]).all()
    assert got["best"][1] == -1 and got["best"][2] == 0
    free = bundles("iv", SSPP_SCENES["iv"], count_static=False)
    assert free.scene.info()["static_contacts"] == 1
    free.memo.update(b.memo)  # the same scene: the same reference
    _, _, r = sspp_case(free, 0, 0)
    assert_not_vacuous(r)


def test_cylcyl_option_reads_zero_without_such_pairs(bundles):
    import sspp_amd as S
    st = [Y.ramp()] + Y.one_type_statics("cylinders")
    b = bundles("plain", (st, [Y.body("mover", (0, 0, 0.3), [Y.geom(Y.BOX, Y.MOVER_BOX, name="m_box")])]))
    knots, ctrl0 = linear_init(CC.START, CC.END, N_CTRL)
    job = S.SsppJob(b.scene, knots, 3, ctrl0, CC.SIGMA, CC.LIMITS, W, seed=SEED, max_batch=B)
    run_sspp(job, B)
    assert job.get_option(S._lib.OPT_CYLCYL) == 0 and not job.config()["cylinder_cylinder"]
    assert job.config()["cylinder_box"]


def test_dropin_sspp_returns_only_reference_feasible_paths(bundles):
    from sspp import _sspp
    b = bundles("i", SSPP_SCENES["i"])
    planner = _sspp.SamplingPathPlanner7(b.path)
    ok, paths = planner.plan(CC.START, CC.END, CC.SIGMA, CC.LIMITS, sample_count=512, check_points=W,
                             init_points=N_CTRL)
    init = _sspp.Spline7()
    assert planner.initializePath(CC.START, CC.END, init, N_CTRL)
    ctrl = O.sample_sspp(init.ctrls().T.copy(), 3, CC.SIGMA, CC.LIMITS, planner.seed, 0, 512)
    r = CC.sspp_reference(b.ref, init.knots(), ctrl, W, D)
    assert not r["near"].any() and ok and MIN_EACH <= int(r["feas"].sum()) <= 512 - MIN_EACH
    idx = np.flatnonzero(r["feas"])
    assert len(paths) == len(idx)
    for s, i in zip(paths, idx):
        np.testing.assert_allclose(s.ctrls().T, ctrl[i], rtol=0, atol=1e-12)


# ------------------------------------------------------------------ crafted threshold poses
OFFSETS = [s * m for m in (1e-9, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3) for s in (1.0, -1.0)]
Q_GEN = R.rot_axis(np.array([0.6, 0.0, 0.8]), 0.9) @ R.rot_axis(np.array([0.0, 1.0, 0.0]), 0.3)
SPACING = np.array([1.0, 0.0, 0.0])  # the families' static cylinders stand 1 m apart


def threshold_scene(fams, rot, thr, margin, mover_quat=None):
    """One static cylinder per family, placed at signed distance `thr` from a mover cylinder whose
    body sits at k * SPACING; returns (statics, bodies, poses): poses[k] = (origin, quat, d)."""
    st, poses = [], []
    for k, f in enumerate(fams):
        T, a1, R1, H1, a2, R2, H2, M1, M2 = R.family_pose(f, R.sd_for_gap(f, thr))
        st.append(CC.post(R2, H2, k * SPACING + rot @ T, _mat_to_quat(rot @ M2), name="s_" + f[0], margin=margin))
        poses.append((k * SPACING, _mat_to_quat(rot @ M1), rot @ f[5]))
    geom_q = (1.0, 0.0, 0.0, 0.0) if mover_quat is None else mover_quat
    mover = Y.body("mover", (0, 0, 0), [CC.mover_cyl(0.05, 0.08, quat=geom_q, margin=margin)])
    return st, [mover], poses


@pytest.mark.parametrize("rot", ["identity", "generic"])
@pytest.mark.parametrize("margin", [0.0, 1e-3, 1e-2])
def test_sspp_score_ctrl_threshold_poses(bundles, margin, rot):
    """score_ctrl on rows of equal control points: the mover cylinder at sd = margin + offset from
    each analytic family's static cylinder, offsets +-{1e-9 .. 1e-3}: feasible iff offset > 0."""
    import sspp_amd as S
    import torch
    fams = R.analytic_families()
    Rm = np.eye(3) if rot == "identity" else Q_GEN
    b = bundles("thr_%s_%g" % (rot, margin), threshold_scene(fams, Rm, margin, margin)[:2])
    rows, want = [], []
    for f, (org, quat, d) in zip(fams, threshold_scene(fams, Rm, margin, margin)[2]):
        for off in OFFSETS:
            if f[0] in R.POSITIVE_ONLY and margin + off <= 0:
                continue
            gap = R.sd_for_gap(f, margin + off) - R.sd_for_gap(f, margin)  # cylinder 2 moved by gap along d
            rows.append(np.concatenate([org - d * gap, quat]))
            want.append(off > 0)
    ctrl = np.repeat(np.array(rows)[:, None, :], N_CTRL, axis=1)
    knots, ctrl0 = linear_init(rows[0], rows[0], N_CTRL)
    for f32, order in ((1, 2), (0, 0)):
        job = S.SsppJob(b.scene, knots, 3, ctrl0, 0.0, CC.LIMITS, W, seed=SEED, max_batch=len(rows))
        job.set_option(S.OPT_F32, f32)
        job.set_option(S.OPT_ORDER, order)
        out = job.alloc(len(rows))
        job.score_ctrl(torch.from_numpy(ctrl).cuda(), 0, out["arc"], out["feasible"], out["best"])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(out["feasible"]).astype(bool), np.array(want))


# scene -> (families, the mover geom's rotation in its body): a yaw-only mover keeps that rotation,
# so the crossed-axes family (cylinder 1 along y) has the mover geom turned by pi / 2 about x
TSP_FAMS = {"vertical": (("parallel_side", "stacked_caps", "rim_rim_diagonal"), None),
            "tilted": (("lying_on_cap", "tilted_on_cap"), None),
            "crossed": (("crossed",), R.rot_axis(np.array([1.0, 0.0, 0.0]), np.pi / 2))}


@pytest.mark.parametrize("name", list(TSP_FAMS))
def test_tsp_score_vias_deep_threshold_poses(bundles, name):
    """score_vias with start = vias = end: the mover's vertical cylinder at sd = -1e-3 + offset from
    vertical static cylinders (the upright kernels) and from tilted ones (the generic kernels), and
    a mover cylinder lying along y across a static one along x (crossed axes, decided by a1 x a2):
    a deep contact, C_nf != 0 and status 0, iff offset < 0; forms 0, 1 and forced generic."""
    import sspp_amd as S
    import torch
    names, geom_rot = TSP_FAMS[name]
    fams = [f for f in R.analytic_families() if f[0] in names]
    assert len(fams) == len(names) and all(np.array_equal(f[1], np.eye(3) if geom_rot is None else geom_rot) for f in fams)
    st, bodies, poses = threshold_scene(fams, np.eye(3), R.DEEP, 0.0,
                                        None if geom_rot is None else _mat_to_quat(geom_rot))
    b = bundles("tsp_thr_" + name, (st, bodies), 1, "mover")
    for f, (org, quat, d) in zip(fams, poses):
        for off in OFFSETS:
            gap = R.sd_for_gap(f, R.DEEP + off) - R.sd_for_gap(f, R.DEEP)
            q = np.concatenate([org - d * gap, [0.0]])
            job = S.TspJob(b.scene, q, q, 1, 8, lo=(-8.0,) * 4, hi=(8.0,) * 4, z_min=-8.0, seed=SEED, max_batch=8)
            for form, gen in ((0, 0), (-1, 0), (0, 1)):
                job.set_option(S.OPT_TSP_FORM, form)
                job.set_option(S.OPT_TSP_GENERIC, gen)
                out = job.alloc(1)
                job.score_vias(torch.from_numpy(q[None, None, :].copy()).cuda(), 0, out["L"], out["Cnf"], out["Cwf"],
                               out["status"], out["cost"], out["best"])
                torch.cuda.synchronize()
                assert (_np(out["Cnf"])[0] != 0.0) == (off < 0) == (_np(out["status"])[0] == 0), (f[0], off, form, gen)


# ------------------------------------------------------------------ TaskSpacePlanner
TSP_B, TSP_K, TSP_CP = 512, 2, 40


def tsp_bundle(bundles, tilted):
    return bundles("tsp_tilted" if tilted else "tsp_upright", CC.tsp_gripper(tilted), 1, "mover")


def every_pair_upright(ref, arg):
    """the host's condition for the closed-form kernels, restated: every moving cylinder and box
    geom unrotated in its body, every static cylinder vertical, every static box turned about z"""
    for g, t in enumerate(ref["geom_type"]):
        if t in (Y.CYLINDER, Y.BOX):
            w, x, y, z = ref["geom_quat"][g]
            if x != 0.0 or y != 0.0 or (ref["geom_body"][g] == arg and z != 0.0):
                return False
    return True


@pytest.mark.parametrize("form", [0, 1, 3, 4])
@pytest.mark.parametrize("tilted", [False, True], ids=["upright", "tilted"])
def test_tsp_cylinder_scenes_match_reference(bundles, tilted, form):
    """A gripper-like mover (a box and a vertical cylinder) among vertical posts — every
    cylinder-box and cylinder-cylinder pair vertical / upright, the condition under which the
    closed-form kernels run (the choice itself is not readable through the ABI; forcing the generic
    kernels must give the same results) — and with one post tilted (the generic kernels).  Status
    equal, L / C_nf / C_wf / cost within 1e-9 of the composed reference on the GPU's via sets."""
    import sspp_amd as S
    import torch
    b = tsp_bundle(bundles, tilted)
    assert every_pair_upright(b.ref, b.arg) == (not tilted)
    mean = np.array([Y.TSP_START + (Y.TSP_END - Y.TSP_START) * (i + 1) / (TSP_K + 1) for i in range(TSP_K)])
    sigma = np.full((TSP_K, 4), 0.15)
    res = []
    for gen in (0, 1):
        job = S.TspJob(b.scene, Y.TSP_START, Y.TSP_END, TSP_K, TSP_CP, mean=mean, sigma=sigma, lo=Y.TSP_LO, hi=Y.TSP_HI,
                       z_min=0.0, seed=SEED, max_batch=TSP_B)
        job.set_option(S.OPT_TSP_FORM, form)
        job.set_option(S.OPT_TSP_GENERIC, gen)
        out = job.alloc(TSP_B, with_vias=True)
        job.sample_score(5, TSP_B, out["L"], out["Cnf"], out["Cwf"], out["status"], out["cost"], out["best"],
                         vias_out=out["vias"])
        torch.cuda.synchronize()
        assert job.get_option(S.OPT_TSP_FORM) == form
        res.append({k: _np(v) for k, v in out.items()})
    for k in res[0]:
        np.testing.assert_array_equal(res[0][k], res[1][k], err_msg=k)
    out = res[0]
    vias = out["vias"]
    vias_o = O.sample_tsp(mean, sigma, Y.TSP_LO, Y.TSP_HI, 0.0, SEED, 5, TSP_B)
    assert np.abs(vias - vias_o).max() <= 1e-12
    key = ("tsp", vias.tobytes())
    if key not in b.memo:
        occ = O.Scene(CC.oracle_copy(b.ref), 1, b.arg)
        pairs = CC.cc_pairs(b.ref, {b.arg})
        b.memo[key] = (pairs, CC.tsp_compose(occ, b.ref, pairs, Y.TSP_START, Y.TSP_END, vias, TSP_CP))
    pairs, (L, Cnf, Cwf, st, cost, deep, near) = b.memo[key]
    keep = ~near
    assert len(pairs) == 3 and (~keep).sum() <= 2
    assert MIN_EACH <= int(st.sum()) <= TSP_B - MIN_EACH
    assert (deep.max((0, 1)) >= 1).all()  # every cylinder-cylinder pair deep at some waypoint
    np.testing.assert_array_equal(out["status"][keep], st[keep])
    for a, o in ((out["L"], L), (out["Cnf"], Cnf), (out["Cwf"], Cwf), (out["cost"], cost)):
        assert np.abs(a - o)[keep].max() <= 1e-9
    if keep.all():
        idx_o, _ = O.tsp_best(cost, st)
        c, idx, cnt = S.decode_best(out["best"])
        assert cnt == int(st.sum()) and idx == (idx_o + 5 if idx_o >= 0 else -1)


def test_ces_plan_group_equals_per_goal_plan(bundles):
    """Two CES iterations of sspp_ces_plan_group for two goals on the gripper scene against each
    goal's own plan: every read() field bit for bit."""
    import sspp_amd as S
    b = tsp_bundle(bundles, False)
    starts = np.array([Y.TSP_START, Y.TSP_START + np.array([0.0, 0.05, 0.05, 0.0])])
    ends = np.array([Y.TSP_END, Y.TSP_END + np.array([0.0, -0.1, 0.05, -0.3])])

    def make():
        return [S.CesPlanner(b.scene, sample_count=256, check_points=40, init_points=3, limits_min=Y.TSP_LO,
                             limits_max=Y.TSP_HI, seed=S.DEFAULT_SEED + g) for g in range(2)]
    solo, group = make(), make()
    for p, st, en in zip(solo, starts, ends):
        p.plan(st, en, iterate=False, iterations=2)
    S.CesPlanner.plan_group(group, starts, ends, iterate=False, iterations=2)
    for g, (a, c) in enumerate(zip(solo, group)):
        ra, rc = a.read(), c.read()
        for k in ra:
            np.testing.assert_array_equal(np.asarray(ra[k]), np.asarray(rc[k]), err_msg="goal %d %s" % (g, k))
    assert sum(p.read()["n_success"] for p in solo) > 0


def test_dropin_tsp_successes_are_reference_collision_free(bundles):
    """_tsp.TaskSpacePlanner.plan on the tilted gripper scene rather than SamplingPathPlanner scene
    (i): the same kinds of geoms (vertical and tilted posts, a plane, a box, a mover that carries a
    cylinder), placed where a yaw-only mover between TSP_START and TSP_END both succeeds and fails."""
    from sspp import _tsp
    b = tsp_bundle(bundles, True)
    p = _tsp.TaskSpacePlanner(b.path, "mover", sample_count=256, check_points=40, limits_min=Y.TSP_LO,
                              limits_max=Y.TSP_HI)
    p.plan(Y.TSP_START, Y.TSP_END, False)
    succ = p.plan(Y.TSP_START, Y.TSP_END, True)
    fail = p.get_failed_path_candidates()
    assert len(succ) >= 1 and len(fail) >= 1
    occ = O.Scene(CC.oracle_copy(b.ref), 1, b.arg)
    pairs = CC.cc_pairs(b.ref, {b.arg})
    vias = np.array([np.asarray(c.via, float).reshape(-1, 4) for c in succ])
    L, Cnf, Cwf, st, cost, deep, near = CC.tsp_compose(occ, b.ref, pairs, Y.TSP_START, Y.TSP_END, vias, 40)
    assert (Cnf[~near] == 0.0).all() and all(c.C_nf == 0.0 for c in succ)
