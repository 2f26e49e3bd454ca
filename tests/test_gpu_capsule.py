"""GPU parity on capsule scenes: k_sspp_c2f / k_sspp_census, k_tsp and its forms, k_tsp_group and
the drop-in modules against the composed reference of tests/capsule_scenes.py (the CPU oracle on
the scene without its capsules + tests/capsule_ref.py on the capsule pairs; the oracle knows no
capsule).  Scenes are authored there; the product loads them as written (some capsules by
`fromto`), the independent reader the same scene with every fromto geom restated explicitly.

Bars: test_gpu_parity.py's for the SamplingPathPlanner (sampled control points bit-equal to the
oracle's, flags equal, arcs within COST_TOL, best record equal), the synthetic scenes' 1e-9 for
TaskSpacePlanner costs.  A candidate whose capsule distance lies within 1e-9 of its threshold at
some waypoint is left out (at most 2 of 2048; none for the seeds used, by the reference alone).
Every case asserts, from the reference alone, that it is not vacuous.
"""
import os

import numpy as np
import pytest

from oracle import mjcf_ref
from oracle import oracle as O
from tests import capsule_scenes as CS
from tests import synth_scenes as Y
from tests.conftest import arc_err
from tests.test_gpu_parity import COST_TOL, SHAPES, _np, linear_init, run_sspp

pytestmark = pytest.mark.gpu

LAUNCH = [(0, 0), (128, 4), (64, 3), (256, 64)]
assert set(LAUNCH) <= set(SHAPES)
B, W, N_CTRL, D = 2048, 64, 10, 7
SEED = 7
MIN_EACH = 16
SSPP_SCENES = {"i": CS.sspp_capsule_mover, "ii": CS.sspp_static_capsules, "iii": CS.sspp_two_geom_mover,
               "iv": CS.sspp_static_contact}
# the capsule pair types of each scene (each must decide some candidate alone)
SSPP_TYPES = {"i": {(0, 3), (2, 3), (3, 3), (3, 6)}, "ii": {(2, 3), (3, 6)}, "iii": {(0, 3), (3, 3), (3, 6)},
              "iv": {(2, 3), (3, 6)}}


class Bundle:
    def __init__(self, root, name, scene, mode, arg, count_static=True):
        import sspp_amd as S
        st, bodies = scene() if callable(scene) else scene
        self.path = os.path.join(root, name + ".xml")
        ref_path = os.path.join(root, name + "_explicit.xml")
        with open(self.path, "w") as f:
            f.write(CS.mjcf(st, bodies))
        with open(ref_path, "w") as f:
            f.write(CS.mjcf(st, bodies, as_explicit=True))
        self.model = S.Model(self.path)
        self.ref = mjcf_ref.load(ref_path)
        if not any("fromto" in g for g in st):
            Y.assert_loaders_agree(self.model.arrays(), self.ref)
        if isinstance(arg, str):
            arg = self.ref["body_names"].index(arg)
        self.mode, self.arg = mode, arg
        self.scene = S.Scene(self.model, mode, arg, count_static=count_static)
        self.memo = {}


@pytest.fixture(scope="module")
def bundles(cuda, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("capsule_scenes"))
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
        knots, ctrl0 = linear_init(CS.START, CS.END, N_CTRL)
        ctrl = O.sample_sspp(ctrl0, 3, CS.SIGMA, CS.LIMITS, SEED, 0, B)
        r = CS.sspp_reference(b.ref, knots, ctrl, W, D)
        for a in [ctrl] + [v for v in r.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        b.memo["sspp"] = (knots, ctrl0, ctrl, r)
    return b.memo["sspp"]


def assert_not_vacuous(b, r, types):
    nf = int(r["feas"].sum())
    assert MIN_EACH <= nf <= B - MIN_EACH, nf
    assert int(r["near"].sum()) <= 2
    dec = CS.deciding_types(b.ref, r)
    assert set(dec) == types and all(n >= 1 for n in dec.values()), dec


def sspp_case(b, nt, g1, order=None):
    import sspp_amd as S
    knots, ctrl0, ctrl, r = sspp_ref(b)
    job = S.SsppJob(b.scene, knots, 3, ctrl0, CS.SIGMA, CS.LIMITS, W, seed=SEED, max_batch=B)
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
    assert job.get_option(S._lib.OPT_CAPSULE) == 1 and job.config()["capsule"]
    assert not job.config()["cylinder_box"] and not job.config()["split"]
    return job, got, r


@pytest.mark.parametrize("nt,g1", LAUNCH)
@pytest.mark.parametrize("case", ["i", "ii", "iii"])
def test_sspp_capsule_scenes_match_reference(bundles, case, nt, g1):
    """(i) a capsule mover against the tilted plane, a sphere, a capsule and a box; (ii) a box and
    a sphere mover geom against static capsules, two of them written with fromto; (iii) a capsule +
    box mover (ONEGEOM false) in a table with box-box pairs: the FP32-filtered scan settles those
    and leaves every capsule pair to FP64."""
    b = bundles(case, SSPP_SCENES[case])
    job, got, r = sspp_case(b, nt, g1)
    assert_not_vacuous(b, r, SSPP_TYPES[case])
    assert job.config()["sampled_pairs"] == b.scene.info()["n_pairs"] == len(Y.moving_pairs(b.ref, D))
    if case == "iii":
        assert job.config()["scan"] == "fp32-filtered"
        types = {tuple(sorted((b.ref["geom_type"][a], b.ref["geom_type"][c]))) for a, c in Y.moving_pairs(b.ref, D)}
        assert (6, 6) in types and (0, 6) in types


@pytest.mark.parametrize("order", [0, 1, 2])
def test_sspp_capsule_scan_orders(bundles, order):
    """Every pair / waypoint scan order (the census kernel runs for order 2) gives the same results."""
    b = bundles("iii", SSPP_SCENES["iii"])
    sspp_case(b, 0, 0, order=order)


def test_sspp_static_capsule_contact(bundles):
    """(iv) a capsule resting in a box, both static: the scene's static contact count is the
    reference's, count_static makes every candidate infeasible, and without it the scene scores
    like (ii) plus the pairs against the resting capsule."""
    import sspp_amd as S
    b = bundles("iv", SSPP_SCENES["iv"])
    ocap = O.Scene(b.ref, 0, D, skip_types=(CS.CAPSULE,))
    want = CS.static_capsule_contacts(b.ref, ocap, {b.ref["body_names"].index("mover")})
    assert want == 1 == b.scene.info()["static_contacts"]
    knots, ctrl0, ctrl, r = sspp_ref(b)
    job = S.SsppJob(b.scene, knots, 3, ctrl0, CS.SIGMA, CS.LIMITS, W, seed=SEED, max_batch=B)
    got = run_sspp(job, B)
    assert np.array_equal(got["ctrl"], ctrl)
    assert not got["feasible"].any() and np.isinf(got["arc"]).all()
    assert got["best"][1] == -1 and got["best"][2] == 0
    free = bundles("iv", SSPP_SCENES["iv"], count_static=False)
    assert free.scene.info()["static_contacts"] == 1
    free.memo.update(b.memo)  # the same scene: the same reference
    _, _, r = sspp_case(free, 0, 0)
    assert_not_vacuous(free, r, SSPP_TYPES["iv"])


def test_capsule_option_reads_zero_without_capsules(bundles):
    import sspp_amd as S
    st = [Y.ramp()] + Y.one_type_statics("spheres")
    b = bundles("plain", (st, [Y.body("mover", (0, 0, 0.3), [Y.geom(Y.BOX, Y.MOVER_BOX, name="m_box")])]))
    knots, ctrl0 = linear_init(CS.START, CS.END, N_CTRL)
    job = S.SsppJob(b.scene, knots, 3, ctrl0, CS.SIGMA, CS.LIMITS, W, seed=SEED, max_batch=B)
    run_sspp(job, B)
    assert job.get_option(S._lib.OPT_CAPSULE) == 0 and not job.config()["capsule"]


def test_dropin_sspp_returns_only_reference_feasible_paths(bundles):
    from sspp import _sspp
    b = bundles("i", SSPP_SCENES["i"])
    planner = _sspp.SamplingPathPlanner7(b.path)
    ok, paths = planner.plan(CS.START, CS.END, CS.SIGMA, CS.LIMITS, sample_count=512, check_points=W,
                             init_points=N_CTRL)
    init = _sspp.Spline7()
    assert planner.initializePath(CS.START, CS.END, init, N_CTRL)
    knots = init.knots()
    ctrl = O.sample_sspp(init.ctrls().T.copy(), 3, CS.SIGMA, CS.LIMITS, planner.seed, 0, 512)
    r = CS.sspp_reference(b.ref, knots, ctrl, W, D)
    assert not r["near"].any() and ok and MIN_EACH <= int(r["feas"].sum()) <= 512 - MIN_EACH
    idx = np.flatnonzero(r["feas"])
    assert len(paths) == len(idx)
    for s, i in zip(paths, idx):
        np.testing.assert_allclose(s.ctrls().T, ctrl[i], rtol=0, atol=1e-12)


# ------------------------------------------------------------------ TaskSpacePlanner
TSP_B, TSP_K = 256, 2
TSP_SCENES = {"capsule_mover": CS.tsp_capsule_mover, "box_mover": CS.tsp_box_mover}


def tsp_bundle(bundles, name):
    return bundles("tsp_" + name, TSP_SCENES[name], 1, "mover")


@pytest.mark.parametrize("form", [-1, 0])
@pytest.mark.parametrize("cp", [40, 65])
@pytest.mark.parametrize("name", list(TSP_SCENES))
def test_tsp_capsule_scenes_match_reference(bundles, name, cp, form):
    """A vertical capsule mover among vertical capsules (the parallel branch: two deep contacts
    from one pair), a tilted capsule, boxes and the floor; a box mover among capsules.  Status
    equal, L / C_nf / C_wf / cost within 1e-9 of the composed reference on the GPU's via sets."""
    import sspp_amd as S
    import torch
    b = tsp_bundle(bundles, name)
    mean = np.array([Y.TSP_START + (Y.TSP_END - Y.TSP_START) * (i + 1) / (TSP_K + 1) for i in range(TSP_K)])
    sigma = np.full((TSP_K, 4), 0.15)
    job = S.TspJob(b.scene, Y.TSP_START, Y.TSP_END, TSP_K, cp, mean=mean, sigma=sigma, lo=Y.TSP_LO, hi=Y.TSP_HI,
                   z_min=0.0, seed=SEED, max_batch=TSP_B)
    job.set_option(S.OPT_TSP_FORM, form)
    out = job.alloc(TSP_B, with_vias=True)
    job.sample_score(5, TSP_B, out["L"], out["Cnf"], out["Cwf"], out["status"], out["cost"], out["best"],
                     vias_out=out["vias"])
    torch.cuda.synchronize()
    vias = _np(out["vias"])
    vias_o = O.sample_tsp(mean, sigma, Y.TSP_LO, Y.TSP_HI, 0.0, SEED, 5, TSP_B)
    assert np.abs(vias - vias_o).max() <= 1e-12
    key = ("tsp", cp, vias.tobytes())
    if key not in b.memo:
        ocap = O.Scene(b.ref, 1, b.arg, skip_types=(CS.CAPSULE,))
        pairs = CS.capsule_pairs(b.ref, {b.arg})
        b.memo[key] = (pairs, CS.tsp_compose(ocap, b.ref, pairs, Y.TSP_START, Y.TSP_END, vias, cp))
    pairs, (L, Cnf, Cwf, st, cost, deep, gap) = b.memo[key]
    # not vacuous: both statuses, every capsule pair deep somewhere, the parallel branch's two
    keep = ~(gap < 1e-9).any(1)
    assert (~keep).sum() <= 2
    assert MIN_EACH <= int(st.sum()) <= TSP_B - MIN_EACH
    assert (deep.max((0, 1)) >= 1).all()
    if name == "capsule_mover":
        par = [k for k, (g1, g2, _) in enumerate(pairs) if b.ref["geom_names"][g1] in ("v0", "v1")]
        assert len(par) == 2 and all(deep[:, :, k].max() == 2 for k in par)
    np.testing.assert_array_equal(_np(out["status"])[keep], st[keep])
    for a, o in ((out["L"], L), (out["Cnf"], Cnf), (out["Cwf"], Cwf), (out["cost"], cost)):
        assert np.abs(_np(a) - o)[keep].max() <= 1e-9
    if keep.all():
        idx_o, _ = O.tsp_best(cost, st)
        c, idx, cnt = S.decode_best(out["best"])
        assert cnt == int(st.sum()) and idx == (idx_o + 5 if idx_o >= 0 else -1)


def test_ces_plan_group_equals_per_goal_plan(bundles):
    """Two CES iterations of sspp_ces_plan_group for two goals on a capsule scene against each
    goal's own plan: every read() field bit for bit."""
    import sspp_amd as S
    b = tsp_bundle(bundles, "capsule_mover")
    starts = np.array([Y.TSP_START, Y.TSP_START + np.array([0.0, 0.05, 0.05, 0.0])])
    ends = np.array([Y.TSP_END, Y.TSP_END + np.array([0.0, -0.1, 0.05, -0.3])])

    def make():
        return [S.CesPlanner(b.scene, sample_count=TSP_B, check_points=40, init_points=3, limits_min=Y.TSP_LO,
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
    from sspp import _tsp
    b = tsp_bundle(bundles, "capsule_mover")
    p = _tsp.TaskSpacePlanner(b.path, "mover", sample_count=TSP_B, check_points=40, limits_min=Y.TSP_LO,
                              limits_max=Y.TSP_HI)
    p.plan(Y.TSP_START, Y.TSP_END, False)
    succ = p.plan(Y.TSP_START, Y.TSP_END, True)
    fail = p.get_failed_path_candidates()
    assert len(succ) >= 1 and len(fail) >= 1
    ocap = O.Scene(b.ref, 1, b.arg, skip_types=(CS.CAPSULE,))
    pairs = CS.capsule_pairs(b.ref, {b.arg})
    vias = np.array([np.asarray(c.via, float).reshape(-1, 4) for c in succ])
    L, Cnf, Cwf, st, cost, deep, gap = CS.tsp_compose(ocap, b.ref, pairs, Y.TSP_START, Y.TSP_END, vias, 40)
    keep = ~(gap < 1e-9).any(1)
    assert (Cnf[keep] == 0.0).all() and all(c.C_nf == 0.0 for c in succ)
