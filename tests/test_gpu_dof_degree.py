"""GPU parity for every (dof, degree) instantiation of k_sspp_c2f / k_sspp_census at its edges.

The kernels are stamped out once per D in {1, 2, 3, 4, 6, 7, 9} and p in {2, 3}; the other GPU
modules run D = 7, p = 3 almost exclusively.  The cases here (tests/dof_degree_cases.py; their
non-vacuity is asserted on the CPU in tests/test_dof_degree_cases.py) take every instantiation
through a collision scene and the sampler, with candidate ids above 2^32, odd and non-multiple-of-4
sampler tails, no perturbed row at all, non-uniform and repeated knots, check-point counts on
both sides of every lanes_for boundary, W = 1, a split multi-step launch away from D = 7, the
largest spline the LDS holds, and the drop-in planners of 3, 6 and 9 dofs.

Bars: sampled control points array_equal to the oracle's, feasibility array_equal, arcs within
1e-12 of the oracle on the control points the GPU returned, the argmin record (count, lowest id
on ties, cost) the oracle's; against arc_ref, max(1e-12, 16 x the oracle's own measured
deviation from arc_ref) relative.
"""
import numpy as np
import pytest

from oracle import mjcf_ref
from oracle import oracle as O
from tests import dof_degree_cases as C
from tests import synth_scenes as Y
from tests.conftest import arc_err
from tests.test_gpu_parity import COST_TOL, _np, linear_init, run_sspp
from tests.test_gpu_synthetic_scenes import assert_sspp_parity

pytestmark = pytest.mark.gpu

SHAPES = [(0, 0), (128, 4), (64, 3)]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("dof_degree")


@pytest.fixture(scope="module")
def scenes(cuda, root):
    """get(name, D): (device scene, oracle scene) of a scene bound to a qpos window of D."""
    import sspp_amd as S
    models, made = {}, {}

    def get(name, D):
        if name not in models:
            path = C.write_scene(root, name)
            models[name] = S.Model(path)
            Y.assert_loaders_agree(models[name].arrays(), mjcf_ref.load(path))
        if (name, D) not in made:
            scene, osc = S.Scene(models[name], 0, D), C.oracle_scene(root, name, D)
            info = scene.info()
            assert info["n_pairs"] == osc.npairs()[0] > 0 and info["static_contacts"] == 0
            made[name, D] = (scene, osc)
        return made[name, D]

    return get


@pytest.fixture(scope="module")
def ref_bar():
    """The device's bar against arc_ref, from the oracle's own deviation over the (d) cases
    (6.2e-16 measured, so 16 x it is below the floor and the bar is 1e-12 relative)."""
    return C.ref_bar(C.oracle_vs_ref())


def problem(D, p, n):
    """(knots, ctrl0, limits): the product's initializePath, which must be the oracle's."""
    s, e, lim = C.ends(D)
    knots, ctrl0 = linear_init(s, e, n, p)
    k_o, c_o = C.init_spline(D, p, n)
    assert np.array_equal(knots, k_o) and np.array_equal(ctrl0, c_o)
    return knots, ctrl0, lim


def sampled_runs(scenes, D, p, n, runs, sampler=0):
    """One job per (nt, g1, arc_all, order) in `runs`, 256 candidates from id 2^40 + 5, each
    against the oracle; returns {run: (job, results)}."""
    import sspp_amd as S
    scene, osc = scenes(C.scene_name(D), D)
    knots, ctrl0, lim = problem(D, p, n)
    sigma = C.sigma_for(D)
    ctrl_o = O.sample_sspp(ctrl0, p, sigma, lim, C.SEED, C.FIRST, C.B, sampler=sampler)
    scored = {a: O.sspp_score(osc, knots, p, ctrl_o, C.W, arc_all=a) for a in {r[2] for r in runs}}
    out = {}
    for run in runs:
        nt, g1, arc_all, order = run
        job = S.SsppJob(scene, knots, p, ctrl0, sigma, lim, C.W, seed=C.SEED, max_batch=C.B, arc_all=arc_all,
                        sampler=sampler)
        job.set_shape(nt, g1)
        if order is not None:
            job.set_option(S.OPT_ORDER, order)
        r = run_sspp(job, C.B, first=C.FIRST)
        arc_o, feas_o = scored[arc_all]
        assert_sspp_parity(r, ctrl_o, arc_o, feas_o, C.FIRST)
        assert np.isinf(r["arc"]).sum() == (0 if arc_all else int((feas_o == 0).sum()))
        assert r["best"][1] >= 2 ** 40  # (the CPU module: at least 8 candidates are feasible)
        out[run] = (job, r)
    return out


# ------------------------------------------------------------------ (a) the matrix with a scene
@pytest.mark.parametrize("D,p,n", C.matrix_cases())
def test_matrix_with_scene(scenes, D, p, n):
    """Every (D, p) with one, two and several perturbed rows, on a scene whose qpos0 rotation
    is not the identity (D = 9: two movers), ids from 2^40 + 5: three launch shapes, arc_all,
    and the three scan orders, which must agree bit for bit.  The default order (2) orders its
    tables by k_sspp_census<D, ., p>'s hit counts (the multi-geom census form here; the
    one-geom form runs in test_split_multistep_launch)."""
    import sspp_amd as S
    runs = [(nt, g1, False, None) for nt, g1 in SHAPES] + [(0, 0, True, None)] + [(0, 0, False, o) for o in (0, 1, 2)]
    got = sampled_runs(scenes, D, p, n, runs)
    job, base = got[0, 0, False, None]
    assert job.get_option(S.OPT_ORDER) == 2 and job.config()["sampler"] == "fp64"
    for order in (0, 1, 2):
        j, r = got[0, 0, False, order]
        assert j.get_option(S.OPT_ORDER) == order
        for k in ("ctrl", "arc", "feasible"):
            np.testing.assert_array_equal(r[k], base[k], err_msg="order %d %s" % (order, k))
        assert r["best"] == base["best"]


# ------------------------------------------------------------------ (b) the FP32 sampler's tails
@pytest.mark.parametrize("D,p,n", C.FP32_CASES)
def test_fp32_sampler_tails(scenes, D, p, n):
    """npert = 1, 3, 6, 7, 18: the last quad of the FP32 sampler writes 1, 3, 2, 3, 2 entries."""
    got = sampled_runs(scenes, D, p, n, [(nt, g1, False, None) for nt, g1 in SHAPES], sampler=O.SAMPLER_FP32)
    job, r = got[0, 0, False, None]
    assert job.config()["sampler"] == "fp32"
    knots, ctrl0, lim = problem(D, p, n)
    assert not np.array_equal(r["ctrl"], O.sample_sspp(ctrl0, p, C.sigma_for(D), lim, C.SEED, C.FIRST, C.B))


# ------------------------------------------------------------------ (c) no perturbed row
@pytest.mark.parametrize("nt,g1", [(0, 0), (64, 64), (128, 4)])
@pytest.mark.parametrize("D,p,n,with_scene", C.nopert_cases())
def test_no_perturbed_row(scenes, D, p, n, with_scene, nt, g1):
    """n <= 2p: rows p .. n - p - 1 are none, so a sampling job with sigma 0.2 has no sample
    item and no own row per candidate; every candidate is the initial spline (feasible by
    construction), all 300 costs tie, and the lowest id — the batch straddles 2^33 — must win
    across workgroups."""
    import sspp_amd as S
    scene, osc = scenes(C.scene_name(D), D) if with_scene else (None, None)
    knots, ctrl0, lim = problem(D, p, n)
    job = S.SsppJob(scene, knots, p, ctrl0, C.NOPERT_SIGMA, lim, C.W, seed=C.SEED, max_batch=C.NOPERT_B)
    job.set_shape(nt, g1)
    r = run_sspp(job, C.NOPERT_B, first=C.NOPERT_FIRST)
    assert all(np.array_equal(c, ctrl0) for c in r["ctrl"])
    assert (r["feasible"] == 1).all()
    assert np.isfinite(r["arc"][0]) and (r["arc"] == r["arc"][0]).all()
    arc_o, feas_o = O.sspp_score(osc, knots, p, ctrl0[None], C.W)
    assert feas_o[0] == 1 and abs(r["arc"][0] - arc_o[0]) <= COST_TOL
    assert r["best"] == (float(r["arc"][0]), C.NOPERT_FIRST, C.NOPERT_B)


# ------------------------------------------------------------------ (d) knots and W, no scene
@pytest.mark.parametrize("D,p,n,kind,W", C.knot_cases())
def test_knots_and_check_points(cuda, ref_bar, D, p, n, kind, W):
    """computeArcLength of 64 random caller splines: uniform, random, repeated and on-grid
    interior knots, Bezier to 13 control points, W on both sides of 64 | 65, 128 | 129,
    192 | 193 and 256 | 257 chords and beyond one chord per lane."""
    import sspp_amd as S
    import torch
    knots, ctrl = C.knot_case_data(D, p, n, kind, W)
    job = S.SsppJob(None, knots, p, ctrl[0], 0.0, np.ones(D), W, max_batch=C.N_SPLINES)
    out = job.alloc(C.N_SPLINES)
    job.score_ctrl(torch.from_numpy(ctrl).cuda(), 0, out["arc"], out["feasible"], out["best"])
    torch.cuda.synchronize()
    arc = _np(out["arc"])
    arc_o, feas_o = O.sspp_score(None, knots, p, ctrl, W)
    print("max |device - oracle| = %.3e" % arc_err(arc, arc_o))
    assert _np(out["feasible"]).all() and feas_o.all()
    assert arc_err(arc, arc_o) <= COST_TOL
    ref = C.arc_ref(knots, p, ctrl, W)
    rel = float(np.max(np.abs(arc.astype(C.LD) - ref) / ref))
    print("max relative |device - arc_ref| = %.3e (bar %.3e)" % (rel, ref_bar))
    assert rel <= ref_bar
    idx_o, best_o = O.argmin(arc_o, feas_o)
    cost, idx, cnt = S.decode_best(out["best"])
    assert idx == idx_o and cnt == C.N_SPLINES and abs(cost - best_o) <= COST_TOL


# ------------------------------------------------------------------ (e) W = 1
@pytest.mark.parametrize("nt,g1", SHAPES)
@pytest.mark.parametrize("D,p", C.W1_CASES)
def test_one_check_point(scenes, root, D, p, nt, g1):
    """check_points = 1 is checkCollision(num_samples = 1): u = 0 and u = 1 only, and an arc
    grid of one point, so arc length 0.  The oracle's scorer refuses W < 2; the expectation is
    its contact count at the two end points."""
    import sspp_amd as S
    import torch
    scene, _ = scenes("window", D)
    knots, ctrl0, ctrl, feas_o = C.w1_expected(root, D, p)
    _, _, lim = C.ends(D)
    for arc_all in (False, True):
        job = S.SsppJob(scene, knots, p, ctrl0, 0.0, lim, 1, max_batch=C.W1_B, arc_all=arc_all)
        job.set_shape(nt, g1)
        out = job.alloc(C.W1_B)
        job.score_ctrl(torch.from_numpy(ctrl).cuda(), C.FIRST, out["arc"], out["feasible"], out["best"])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(out["feasible"]), feas_o)
        want = np.where((feas_o == 1) | arc_all, 0.0, np.inf)
        np.testing.assert_array_equal(_np(out["arc"]), want)
        assert S.decode_best(out["best"]) == (0.0, C.FIRST + int(np.flatnonzero(feas_o)[0]), int(feas_o.sum()))


# ------------------------------------------------------------------ (f) split launch, D != 7
@pytest.mark.parametrize("name", ["window_one", "window_one_nocyl"])
@pytest.mark.parametrize("D,p", C.SPLIT_CASES)
def test_split_multistep_launch(scenes, D, p, name):
    """16 steps x 1024 candidates in one launch (the throughput shape), twice back to back, the
    ids crossing 2^32 at step 3: every step's feasibility, arcs and argmin record against the
    oracle.  A launch splits only over a one-geom table without cylinder-box pairs:
    window_one keeps window's cylinder, so the library reports a cylinder-box table and does not
    split it (its settle step decides those pairs); window_one_nocyl is the same scene without
    the cylinder and must split, with no survivor lost.  Both are one-geom movers, so their
    default hit order comes from the one-geom form of k_sspp_census<D, 1, p>."""
    import sspp_amd as S
    import torch
    scene, osc = scenes(name, D)
    knots, ctrl0, lim = problem(D, p, C.SPLIT_N)
    sigma, steps, B = C.sigma_for(D), C.SPLIT_STEPS, C.SPLIT_B
    job = S.SsppJob(scene, knots, p, ctrl0, sigma, lim, C.W, seed=C.SEED, max_batch=B)
    arcs = [torch.empty(steps * B, dtype=torch.float64, device="cuda")]
    feas = [torch.empty(steps * B, dtype=torch.uint8, device="cuda")]
    ex = S.SsppSteps([job], [torch.cuda.current_stream()], B, arcs, feas, steps_per_launch=steps)
    best = torch.zeros((steps, 4), dtype=torch.int64, device="cuda")
    mixed = 0
    for rep in range(2):
        ex.enqueue(steps, C.SPLIT_FIRST + rep * steps * B, B, best)
        torch.cuda.synchronize()
        cfg = job.config()
        assert cfg["shape"] == "128x4" and cfg["pair_order"] == "hit"
        assert cfg["cylinder_box"] == (name == "window_one")
        assert job.get_option(S._lib.OPT_LAST_SPLIT) == (0 if cfg["cylinder_box"] else 1)
        arc, fe, got = arcs[0].cpu().numpy(), feas[0].cpu().numpy(), best.cpu()
        for i in range(steps):
            f0 = C.SPLIT_FIRST + (rep * steps + i) * B
            ctrl_o = O.sample_sspp(ctrl0, p, sigma, lim, C.SEED, f0, B)
            arc_o, feas_o = O.sspp_score(osc, knots, p, ctrl_o, C.W)
            np.testing.assert_array_equal(fe[i * B:(i + 1) * B], feas_o)
            assert arc_err(arc[i * B:(i + 1) * B], arc_o) <= COST_TOL
            k, best_o = O.argmin(arc_o, feas_o)
            cost, idx, cnt = S.decode_best(got[i])
            assert idx == (f0 + k if k >= 0 else -1) and cnt == int(feas_o.sum()), (rep, i)
            if k >= 0:
                assert abs(cost - best_o) <= COST_TOL
            mixed += int(C.MIN_EACH <= cnt <= B - C.MIN_EACH)
    assert mixed == 2 * steps  # both outcomes in every step
    assert job.get_option(S._lib.OPT_SPLIT_LOST) == 0


# ------------------------------------------------------------------ (g) the LDS limit
@pytest.mark.parametrize("p", C.DEGREES)
def test_lds_limit(cuda, ref_bar, p):
    """The largest D = 9 spline a job takes (sspp_job_create_sspp refuses what the latency shape
    could not launch: SSPP_E_UNSUPPORTED, "too large for LDS"), found by bisection.  At that n
    every launch shape either meets the bars of (d) or is refused naming the LDS; n + 1 is
    refused at creation."""
    import sspp_amd as S
    import torch
    D, W, nb = 9, 65, 8
    created = [0]

    def knots_of(n):
        return C.knot_vector(n, p, "uniform", None)

    def create(n):
        created[0] += 1
        try:
            return S.SsppJob(None, knots_of(n), p, np.zeros((n, D)), 0.0, np.ones(D), W, max_batch=nb)
        except S.SsppError as e:
            assert "(-5)" in str(e) and "too large for LDS" in str(e), str(e)
            return None

    lo, hi = p + 1, 1024  # lo is accepted (every other test's size); hi must not be
    assert create(hi) is None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if create(mid) is not None else (lo, mid)
    assert created[0] <= 12
    n = lo
    print("largest n at D = 9, p = %d: %d" % (p, n))
    assert n >= 13 and create(n + 1) is None  # (13: the largest spline of the other cases)
    knots = knots_of(n)
    ctrl = np.random.default_rng([9, p]).normal(0.0, 1.0, size=(nb, n, D))
    arc_o, feas_o = O.sspp_score(None, knots, p, ctrl, W)
    ref = C.arc_ref(knots, p, ctrl, W)
    ran = []
    for nt, g1 in [(0, 0), (64, 64), (128, 4), (256, 16)]:
        job = create(n)
        job.set_shape(nt, g1)
        out = job.alloc(nb)
        for v in out.values():
            v.fill_(0)
        try:
            job.score_ctrl(torch.from_numpy(ctrl).cuda(), 0, out["arc"], out["feasible"], out["best"])
        except S.SsppError as e:
            assert "LDS" in str(e), str(e)
            torch.cuda.synchronize()
            assert not _np(out["arc"]).any() and not _np(out["best"]).any()  # nothing partial
            continue
        torch.cuda.synchronize()
        ran.append((nt, g1))
        arc = _np(out["arc"])
        assert _np(out["feasible"]).all() and arc_err(arc, arc_o) <= COST_TOL
        assert float(np.max(np.abs(arc.astype(C.LD) - ref) / ref)) <= ref_bar
        idx_o, best_o = O.argmin(arc_o, feas_o)
        cost, idx, cnt = S.decode_best(out["best"])
        assert idx == idx_o and cnt == nb and abs(cost - best_o) <= COST_TOL
    print("shapes that ran:", ran)
    assert (0, 0) in ran  # what creation promised


# ------------------------------------------------------------------ (h) the drop-in modules
@pytest.mark.parametrize("N", [3, 6, 9])
def test_dropin_other_dofs_match_oracle(cuda, root, N):
    """SamplingPathPlanner{3,6,9}.plan with three perturbed rows: the returned paths are exactly
    the oracle's feasible candidates on the planner's seed, in candidate order, bit for bit."""
    from sspp import _sspp
    planner = getattr(_sspp, "SamplingPathPlanner%d" % N)(C.write_scene(root, C.scene_name(N)))
    assert planner.seed == C.DROPIN_SEED
    start, end, lim = C.ends(N)
    sigma = C.sigma_for(N)
    ok, paths = planner.plan(start, end, sigma, lim, **C.DROPIN)
    n, W, B = C.DROPIN["init_points"], C.DROPIN["check_points"], C.DROPIN["sample_count"]
    init = getattr(_sspp, "Spline%d" % N)()
    assert planner.initializePath(start, end, init, n)
    knots, ctrl0 = C.init_spline(N, 3, n)
    assert np.array_equal(init.knots(), knots) and np.array_equal(init.ctrls().T, ctrl0)
    ctrl = O.sample_sspp(ctrl0, 3, sigma, lim, planner.seed, 0, B)
    arc, feas = O.sspp_score(C.oracle_scene(root, C.scene_name(N), N), knots, 3, ctrl, W)
    ids = np.flatnonzero(feas)
    assert C.MIN_EACH <= len(ids) <= B - C.MIN_EACH
    assert list(planner.last_feasible_ids) == list(ids)
    assert len(paths) == len(ids) and ok == bool(len(ids))
    for s, i in zip(paths, ids):
        assert np.array_equal(s.ctrls().T, ctrl[i]) and np.array_equal(s.knots(), knots)
    idx, best = O.argmin(arc, feas)
    assert planner.last_best_index == idx and abs(planner.last_best_cost - best) <= COST_TOL
    assert np.array_equal(planner.get_ctrl_pts().T, ctrl[idx])


# ------------------------------------------------------------------ sspp_sample_ctrl_host
@pytest.mark.parametrize("p", C.DEGREES)
@pytest.mark.parametrize("D", C.DOFS)
def test_host_sampler_matches_oracle(cuda, D, p):
    """sspp_sample_ctrl_host (sampleWithNoise for host callers; it samples through a device job
    without a scene) against O.sample_sspp for every (D, p), one perturbed row, ids above 2^32."""
    import ctypes as Ct
    from sspp_amd import _lib
    n = 2 * p + 1
    knots, ctrl0, lim = problem(D, p, n)
    sigma = C.sigma_for(D)
    out = np.zeros((C.B, n, D))
    dp = lambda a: a.ctypes.data_as(Ct.POINTER(Ct.c_double))  # noqa: E731
    _lib.check(_lib.lib().sspp_sample_ctrl_host(dp(knots), p, dp(ctrl0), n, D, sigma, dp(lim), C.SEED, C.FIRST,
                                                C.B, dp(out)), "sspp_sample_ctrl_host")
    want = O.sample_sspp(ctrl0, p, sigma, lim, C.SEED, C.FIRST, C.B)
    assert np.array_equal(out, want)
    assert (want[:, p] != ctrl0[p]).all()  # the one perturbed row moved, in every entry
    assert np.array_equal(want[:, :p], np.repeat(ctrl0[None, :p], C.B, axis=0))
