"""GPU parity at the contact thresholds: the device kernels against the CPU reference on the
crafted poses of tests/boundary_poses.py — every pair type a known 1e-12 .. 1e-3 m on either side
of dist < margin (margins 0, 1e-3, 1e-2) or of the deep threshold dist < -1e-3, at identity,
yaw-only, generic, barely tilted and unnormalised quaternions.

A candidate whose control rows all equal one pose evaluates to that pose at every waypoint, so a
feasibility flag or a TaskSpacePlanner cost is decided by that one pose: the FP32 filter's
certified bands (v_rsq_f32 / v_sqrt_f32 on the device), the culls' pads, the deferred
cylinder-box and capsule settle, the survivors' hull masks on a zero-extent hull and the
TaskSpacePlanner kernels' narrowphase variants each have to get the pose right on their own.

The bars are test_gpu_parity.py's: feasibility and the argmin record equal, arcs and costs within
COST_TOL, against O.sspp_score / O.tsp_score (the composed reference of tests/capsule_scenes.py
where the scene holds a capsule) on the same control points and vias.  Every pose is compared,
the |off| = 1e-12 ones for whatever the reference says.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import boundary_poses as BP
from tests import capsule_scenes as CS
from tests import synth_scenes as Y
from tests.conftest import arc_err
from tests.test_gpu_parity import COST_TOL, _np, linear_init
from tests.test_gpu_synthetic_scenes import LAUNCH

pytestmark = pytest.mark.gpu

W, N_CTRL, D = 8, 10, 7
SEED = 7
# the jobs' own initial spline spans the whole scene, so the sampled-candidate table the library
# reports on (SSPP_OPT_NPAIRS, _CYLBOX, _CAPSULE) is the full table that score_ctrl scans
SPAN_START = np.array([-7.5, -7.5, -1.0, 1, 0, 0, 0])
SPAN_END = np.array([7.5, 7.5, 7.5, 1, 0, 0, 0])
LIMITS = np.ones(7)


class Bundle:
    """One scene on the device and on the reference side."""

    def __init__(self, root, name, scene, mode, arg):
        import sspp_amd as S
        self.path, ref_path = BP.write_scene(root, name, scene)
        self.model = S.Model(self.path)
        self.r = BP.Ref(ref_path, mode, arg)
        Y.assert_loaders_agree(self.model.arrays(), self.r.ref)   # (no fromto geom in these scenes)
        self.scene = S.Scene(self.model, mode, arg)
        info = self.scene.info()
        assert info["n_pairs"] == self.r.full.npairs()[0] and info["static_contacts"] == 0
        self.n_pairs = info["n_pairs"]
        self.memo = {}


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("boundary_scenes"))
    made = {}

    def sspp(kind, margin, table):
        key = (kind, margin, table)
        if key not in made:
            made[key] = Bundle(root, "bp_%s_m%g_%s" % key, BP.sspp_scene(kind, margin, table), 0, D)
        return made[key]

    def tsp(name):
        if name not in made:
            made[name] = Bundle(root, "bp_tsp_%s" % name, BP.tsp_scene(name), 1, "mover")
        return made[name]

    return dict(root=root, sspp=sspp, tsp=tsp)


# ------------------------------------------------------------------ SamplingPathPlanner
def candidates(P, variant):
    """[n, N_CTRL, 7] control rows per pose.  "equal": every row the pose.  "approach": row 0 the
    pose, every other row the pose moved 1 m back along d (P["back"] where the set's cases write
    their own qpos rows); "mirrored": the pose in the last row."""
    q = P["q"]
    ctrl = np.repeat(q[:, None, :], N_CTRL, axis=1).copy()
    if variant != "equal":
        if "back" in P:
            back = P["back"]
        else:
            back = q.copy()
            back[:, :3] += P["d"]
        ctrl[:] = back[:, None, :]
        ctrl[:, 0 if variant == "approach" else -1] = q
    return ctrl


def reference_score(b, knots, ctrl):
    """(arc, feasible) of the reference: the oracle, composed where the scene has capsules."""
    if b.r.has_capsule:
        r = CS.sspp_reference(b.r.ref, knots, ctrl, W, D)
        return r["arc"], r["feas"]
    return O.sspp_score(b.r.full, knots, 3, ctrl, W)


def sspp_reference(world, b, kind, margin, knots, variant):
    """Once per (scene, variant): candidates and their reference scores.  A capsule scene's
    composed reference is computed on the small table (it walks every waypoint in numpy; the
    fillers of the larger tables never touch: test_boundary_poses.test_scene_tables)."""
    src = world["sspp"](kind, margin, "small") if b.r.has_capsule else b
    key = ("ref", variant)
    if key not in src.memo:
        _, cases, P = BP.sspp_set(world["root"], kind, margin)
        ctrl = candidates(P, variant)
        arc, feas = reference_score(src, knots, ctrl)
        for a in (ctrl, arc, feas):
            a.setflags(write=False)
        # not vacuous, from the reference alone: the flag follows the offset's sign wherever the
        # generator guarantees it, so both outcomes occur for every pair type of the scene
        sure = np.abs(P["off"]) >= BP.FLOOR
        assert np.array_equal(feas[sure] == 0, P["off"][sure] < 0)
        for pair in {c["pair"] for c in cases}:
            mine = np.array([cases[k]["pair"] == pair for k in P["case"]])
            assert 0 < int(feas[mine].sum()) < int(mine.sum())
        if variant != "equal":
            # waypoint 0 (W for the mirrored variant) is the only one in contact: the others lie
            # farther along d, the nearest of them (index 1 / W - 1) clear for every candidate
            # and, on a sample, all of them
            at, nxt = (0, 1) if variant == "approach" else (W, W - 1)
            for i, c in enumerate(ctrl):
                pts = range(W + 1) if i % 10 == 0 else (nxt,)
                for k in pts:
                    n = src.r.contacts(O.spline_eval(knots, 3, c, k / W))[0]
                    assert (n > 0) == (k == at and feas[i] == 0), (i, k)
        src.memo[key] = (ctrl, arc, feas)
    return src.memo[key]


def run_score_ctrl(b, knots, ctrl0, ctrl, nt, g1, f32, order, limits=LIMITS):
    import sspp_amd as S
    import torch
    n = len(ctrl)
    job = S.SsppJob(b.scene, knots, 3, ctrl0, 0.0, limits, W, seed=SEED, max_batch=n)
    job.set_shape(nt, g1)
    job.set_option(S.OPT_F32, f32)
    job.set_option(S.OPT_ORDER, order)
    out = job.alloc(n)
    job.score_ctrl(torch.from_numpy(np.array(ctrl)).cuda(), 0, out["arc"], out["feasible"], out["best"])
    torch.cuda.synchronize()
    return job, _np(out["arc"]), _np(out["feasible"]), S.decode_best(out["best"])


def assert_parity(arc, feas, best, arc_o, feas_o, first=0):
    np.testing.assert_array_equal(feas, feas_o)
    assert arc_err(arc, arc_o) <= COST_TOL
    idx_o, best_o = O.argmin(arc_o, feas_o)
    cost, idx, cnt = best
    assert cnt == int(feas_o.sum())
    assert idx == (idx_o + first if idx_o >= 0 else -1)
    if idx_o >= 0:
        assert abs(cost - best_o) <= COST_TOL


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("f32", [1, 0])
@pytest.mark.parametrize("nt,g1", LAUNCH)
@pytest.mark.parametrize("table", list(BP.TABLES))
@pytest.mark.parametrize("kind", BP.SSPP_KINDS)
def test_sspp_boundary_poses(world, kind, table, nt, g1, f32, order):
    """score_ctrl on the boundary poses of one mover kind, at every margin: all rows equal (the
    zero-extent hull), the approach variant (the hit at u = 0 only, wherever the job's waypoint
    order puts it) and its mirror (u = 1 only).  Per launch the library's reported scan, pair
    count and the cylinder-box / capsule flags (so the deferred settle is known to have run)."""
    knots, ctrl0 = linear_init(SPAN_START, SPAN_END, N_CTRL)
    for margin in BP.MARGINS:
        b = world["sspp"](kind, margin, table)
        types = {tuple(sorted((b.r.ref["geom_type"][a], b.r.ref["geom_type"][c]))) for a, c in Y.moving_pairs(b.r.ref, D)}
        for variant in ("equal", "approach", "mirrored"):
            ctrl, arc_o, feas_o = sspp_reference(world, b, kind, margin, knots, variant)
            job, arc, feas, best = run_score_ctrl(b, knots, ctrl0, ctrl, nt, g1, f32, order)
            assert_parity(arc, feas, best, arc_o, feas_o)
            cfg = job.config()
            want_scan = Y.expected_scan(b.r.ref, D) if f32 else "fp64"
            assert cfg["scan"] == want_scan == ("fp32-filtered" if f32 and table != "big" else "fp64")
            assert cfg["sampled_pairs"] == b.n_pairs == {"small": b.n_pairs, "hull": 12, "big": 65}[table]
            assert cfg["pair_order"] == {0: "scene", 1: "gap", 2: "hit"}[order] and not cfg["split"]
            assert cfg["cylinder_box"] == ((BP.CYLINDER, BP.BOX) in types)
            assert cfg["capsule"] == any(BP.CAPSULE in t for t in types) == b.r.has_capsule


SAMPLE_B = 4
SAMPLE_SIGMA = 1e-6


def sampled_around(b, P, score, dof=D, limits=LIMITS):
    """sample_score with sigma = 1e-6 and start = end = each pose of P: one job per pose (the
    initial spline is the job's), a few candidates each; sampled control points bit-equal to the
    oracle's, feasibility for whatever the reference (score(knots, ctrl) -> (arc, feasible)) says
    of them; both outcomes occur.  Returns the jobs."""
    import sspp_amd as S
    import torch
    n = len(P["q"])
    arc = torch.empty(n * SAMPLE_B, dtype=torch.float64, device="cuda")
    feas = torch.empty(n * SAMPLE_B, dtype=torch.uint8, device="cuda")
    ctrl = torch.empty((n * SAMPLE_B, N_CTRL, dof), dtype=torch.float64, device="cuda")
    best = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    jobs, ctrl_o = [], np.empty((n * SAMPLE_B, N_CTRL, dof))
    knots = None
    for i, q in enumerate(P["q"]):
        knots, ctrl0 = linear_init(q, q, N_CTRL)
        job = S.SsppJob(b.scene, knots, 3, ctrl0, SAMPLE_SIGMA, limits, W, seed=SEED, max_batch=SAMPLE_B)
        s = slice(i * SAMPLE_B, (i + 1) * SAMPLE_B)
        job.sample_score(i * SAMPLE_B, SAMPLE_B, arc[s], feas[s], best[i], ctrl_out=ctrl[s])
        jobs.append(job)
        ctrl_o[s] = O.sample_sspp(ctrl0, 3, SAMPLE_SIGMA, limits, SEED, i * SAMPLE_B, SAMPLE_B)
    torch.cuda.synchronize()
    assert np.array_equal(_np(ctrl), ctrl_o)
    arc_o, feas_o = score(knots, ctrl_o)
    assert 0 < int(feas_o.sum()) < len(feas_o)
    np.testing.assert_array_equal(_np(feas), feas_o)
    assert arc_err(_np(arc), arc_o) <= COST_TOL
    for i in range(0, n, 7):
        s = slice(i * SAMPLE_B, (i + 1) * SAMPLE_B)
        assert_parity(_np(arc[s]), _np(feas[s]), S.decode_best(best[i]), arc_o[s], feas_o[s], first=i * SAMPLE_B)
    return jobs


@pytest.mark.parametrize("margin", BP.MARGINS)
@pytest.mark.parametrize("kind", BP.SSPP_KINDS)
def test_sspp_sampled_around_boundary_poses(world, kind, margin):
    """sample_score around every boundary pose (sampled_around): the kernel's own sampler and its
    FP32 copies feed the scan."""
    b = world["sspp"](kind, margin, "hull")
    _, cases, P = BP.sspp_set(world["root"], kind, margin)
    src = world["sspp"](kind, margin, "small") if b.r.has_capsule else b
    jobs = sampled_around(b, P, lambda knots, ctrl: reference_score(src, knots, ctrl))
    # each job's sampled table is the pairs its candidates can reach: it must keep the target pair
    # of a touching pose, and may drop every pair of a clear one (then the scan has nothing to
    # filter and reports fp64)
    for i in range(0, len(jobs), 3):
        cfg = jobs[i].config()
        assert 0 <= cfg["sampled_pairs"] <= 12 and cfg["pair_order"] == "hit"
        assert cfg["scan"] == ("fp32-filtered" if cfg["sampled_pairs"] else "fp64")
        if P["off"][i] <= -BP.FLOOR:
            assert cfg["sampled_pairs"] >= 1, i


# ------------------------------------------------------------------ TaskSpacePlanner
# (form, rep): SSPP_OPT_TSP_REP only reaches form 3
TSP_FORMS = [(-1, -1), (0, -1), (3, -1), (3, 2), (4, -1)]


def tsp_reference(b, q, K, cp):
    """The reference's (L, C_nf, C_wf, status, cost) of the candidates start = vias = end = q[i]."""
    out = []
    for x in q:
        vias = np.repeat(x[None, None, :], K, axis=1)
        if b.r.has_capsule:
            out.append([v[0] for v in CS.tsp_compose(b.r.oscene, b.r.ref, b.r.cap_pairs, x, x, vias, cp)[:5]])
        else:
            out.append([v[0] for v in O.tsp_score(b.r.full, x, x, vias, cp)])
    return [np.array(col) for col in zip(*out)]


@pytest.mark.parametrize("cp", [8, 40])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("name", BP.TSP_SCENES)
def test_tsp_boundary_poses(world, name, deep, K, cp):
    """score_vias with start = vias = end = a boundary pose (one job per pose: start and end are
    the job's), in every kernel form the table allows (-1, 0, 3, 4), with the generic narrowphase
    forced or not and two sub-batch settings: status and the argmin record equal, L / C_nf / C_wf /
    cost within COST_TOL (relative above 1), the last launch's form as asked.  A flipped deep
    contact moves C_nf by far more than the tolerance (asserted from the reference)."""
    import sspp_amd as S
    import torch
    b = world["tsp"](name)
    assert b.n_pairs <= 8
    _, cases, P = BP.tsp_set(world["root"], name, deep)
    key = ("tsp", deep, K, cp)
    if key not in b.memo:
        b.memo[key] = tsp_reference(b, P["q"], K, cp)
    L, Cnf, Cwf, st, cost = b.memo[key]
    sure = np.abs(P["off"]) >= BP.FLOOR
    if deep:
        assert np.array_equal(Cnf[sure] != 0.0, P["off"][sure] < 0) and np.array_equal(st == 1, Cnf == 0.0)
        assert np.abs(Cnf[Cnf != 0.0]).min() > 1e3 * COST_TOL * max(1.0, np.abs(Cnf).max())
    else:
        # a contact shallower than 1e-3 costs nothing; off = -1e-3 along d is the deep threshold
        # itself for a head-on approach, and is compared for whatever the reference says
        shallow = P["off"] > -1e-3
        assert (Cnf[shallow] == 0.0).all() and (st[shallow] == 1).all()
    n = len(P["q"])
    cfgs = [(form, rep, gen) for form, rep in TSP_FORMS for gen in (0, 1)]
    f64 = lambda: torch.empty((len(cfgs), n), dtype=torch.float64, device="cuda")  # noqa: E731
    oL, oCnf, oCwf, ocost = f64(), f64(), f64(), f64()
    ost = torch.empty((len(cfgs), n), dtype=torch.uint8, device="cuda")
    obest = torch.zeros((len(cfgs), n, 4), dtype=torch.int64, device="cuda")
    vias = torch.from_numpy(np.repeat(P["q"][:, None, :], K, axis=1).copy()).cuda()
    jobs = []
    for i, q in enumerate(P["q"]):
        job = S.TspJob(b.scene, q, q, K, cp, lo=(-8.0,) * 4, hi=(8.0,) * 4, z_min=0.0, seed=SEED, max_batch=4096)
        jobs.append(job)
        for c, (form, rep, gen) in enumerate(cfgs):
            job.set_option(S.OPT_TSP_FORM, form)
            job.set_option(S.OPT_TSP_REP, rep)
            job.set_option(S.OPT_TSP_GENERIC, gen)
            job.score_vias(vias[i:i + 1], i, oL[c, i:i + 1], oCnf[c, i:i + 1], oCwf[c, i:i + 1], ost[c, i:i + 1],
                           ocost[c, i:i + 1], obest[c, i])
            # one candidate: -1 picks the pair split (form 1); 3 and 4 apply (a box-box pair, <= 8 pairs)
            assert job.get_option(S.OPT_TSP_FORM) == (1 if form < 0 else form), (form, rep, gen)
            if form == 3 and rep > 0:
                assert job.get_option(S.OPT_TSP_REP) == rep
    torch.cuda.synchronize()
    for c, cfg in enumerate(cfgs):
        np.testing.assert_array_equal(_np(ost[c]), st, err_msg=str(cfg))
        for got, want in ((oL, L), (oCnf, Cnf), (oCwf, Cwf), (ocost, cost)):
            assert (np.abs(_np(got[c]) - want) <= COST_TOL * np.maximum(1.0, np.abs(want))).all(), cfg
        rec = _np(obest[c])
        for i in range(0, n, 3):
            _, idx, cnt = S.decode_best(rec[i])
            assert cnt == int(st[i]) and idx == (i if st[i] else -1), (cfg, i)
