"""GPU parity on synthetic scenes: the device kernels vs the CPU oracle where the three shipped
scenes never take them — spheres, a tilted and offset plane, static and tilted cylinders, pair
tables of 64 / 65 / 72 pairs, statics at the edges of the FP32 filter's certified range, a second
mover (D = 9) and a window that cuts the quaternion (D = 6), and TaskSpacePlanner tables that are
non-upright, all-vertical-cylinder or carry a sphere.

The scenes are authored in tests/synth_scenes.py and written to a temporary directory; each is
loaded by the product's loader (device) and by the independent reader (oracle), and the two must
agree.  The bars are test_gpu_parity.py's: sampled control points bit-equal, feasibility and the
argmin record equal, arcs within 1e-12; TaskSpacePlanner costs within 1e-9.  Every case also
asserts, from the oracle alone, that it is not vacuous (both outcomes occur and the primitive or
pair it targets decides some candidates), and the dispatch fact it targets as the library reports
it (scan kind, split flag, pair count, cylinder-box flag, TaskSpacePlanner form).
"""
import os

import numpy as np
import pytest

from oracle import mjcf_ref
from oracle import oracle as O
from tests import synth_scenes as Y
from tests.conftest import arc_err
from tests.test_gpu_parity import COST_TOL, SHAPES, _np, linear_init, run_sspp

pytestmark = pytest.mark.gpu

LAUNCH = [(0, 0), (128, 4), (64, 3), (256, 64)]
assert set(LAUNCH) <= set(SHAPES)
B, W, N_CTRL = 2048, 64, 10
SEED = 7
MIN_EACH = 16  # candidates of either outcome a case needs, or its parity says little


class Bundle:
    """One synthetic scene on both sides, with the oracle results computed for it so far."""

    def __init__(self, path, mode, arg):
        import sspp_amd as S
        self.path = path
        self.model = S.Model(path)
        self.ref = mjcf_ref.load(path)
        Y.assert_loaders_agree(self.model.arrays(), self.ref)
        if isinstance(arg, str):
            assert self.model.body_id(arg) == self.ref["body_names"].index(arg)
            arg = self.ref["body_names"].index(arg)
        self.mode, self.arg = mode, arg
        self.scene = S.Scene(self.model, mode, arg)
        self.oscene = O.Scene(self.ref, mode, arg)
        info = self.scene.info()
        assert info["n_pairs"] == self.oscene.npairs()[0] and info["static_contacts"] == 0
        self.memo = {}

    def reduced(self, off=(), skip_types=()):
        """The oracle scene without some geoms (by index) or geom types."""
        key = ("reduced", tuple(off), tuple(skip_types))
        if key not in self.memo:
            self.memo[key] = O.Scene(Y.with_geoms_off(self.ref, off), self.mode, self.arg, skip_types=skip_types)
        return self.memo[key]

    def named(self, prefix):
        return Y.geoms_named(self.ref, prefix)


@pytest.fixture(scope="module")
def bundles(cuda, tmp_path_factory):
    """get(name, xml, mode, arg): the scene `name`, written and loaded once per module."""
    root = tmp_path_factory.mktemp("synthetic_scenes")
    made = {}

    def get(name, xml, mode=0, arg=7):
        key = (name, mode, arg)
        if key not in made:
            path = os.path.join(str(root), name + ".xml")
            if not os.path.exists(path):
                with open(path, "w") as f:
                    f.write(xml() if callable(xml) else xml)
            made[key] = Bundle(path, mode, arg)
        return made[key]

    return get


# ------------------------------------------------------------------ SamplingPathPlanner helpers
def oracle_sample_score(b, knots, ctrl0, sigma, limits, first=0, n=B, arc_all=False, seed=SEED):
    """The oracle's candidates and their scores, once per (scene, job)."""
    key = ("sspp", ctrl0.tobytes(), sigma, np.asarray(limits).tobytes(), first, n, arc_all, seed)
    if key not in b.memo:
        ctrl = O.sample_sspp(ctrl0, 3, sigma, limits, seed, first, n)
        arc, feas = O.sspp_score(b.oscene, knots, 3, ctrl, W, arc_all=arc_all)
        for a in (ctrl, arc, feas):
            a.setflags(write=False)
        b.memo[key] = (ctrl, arc, feas)
    return b.memo[key]


def oracle_feasible(b, knots, ctrl, off=(), skip_types=()):
    """Feasibility of `ctrl` in the scene without some geoms / types (non-vacuity conditions)."""
    key = ("feas", ctrl.tobytes(), tuple(off), tuple(skip_types))
    if key not in b.memo:
        b.memo[key] = O.sspp_score(b.reduced(off, skip_types), knots, 3, np.ascontiguousarray(ctrl), W)[1]
    return b.memo[key]


def assert_mixed(b, knots, ctrl, feas_o, types):
    """The case's condition, from the oracle alone: at least MIN_EACH feasible and MIN_EACH
    infeasible candidates, and every geom type in `types` decides some candidate (skipping it
    frees at least one)."""
    nf = int(feas_o.sum())
    assert MIN_EACH <= nf <= len(feas_o) - MIN_EACH, nf
    for t in types:
        freed = int(oracle_feasible(b, knots, ctrl, skip_types=(t,)).sum()) - nf
        assert freed >= 1, (t, freed)


def assert_sspp_parity(r, ctrl_o, arc_o, feas_o, first=0):
    assert np.array_equal(r["ctrl"], ctrl_o)  # so the oracle scored what the GPU scored
    np.testing.assert_array_equal(r["feasible"], feas_o)
    assert arc_err(r["arc"], arc_o) <= COST_TOL
    idx_o, best_o = O.argmin(arc_o, feas_o)
    cost, idx, cnt = r["best"]
    assert cnt == int(feas_o.sum())
    assert idx == (idx_o + first if idx_o >= 0 else -1)
    if idx_o >= 0:
        assert abs(cost - best_o) <= COST_TOL


def sample_case(b, start, end, sigma, limits, nt, g1, first=0, arc_all=False, order=None):
    """One sample_score launch of B candidates against the oracle; returns the job and both sides.
    order: SSPP_OPT_ORDER for the job's pair table (None: the library's choice)."""
    import sspp_amd as S
    knots, ctrl0 = linear_init(start, end, N_CTRL)
    job = S.SsppJob(b.scene, knots, 3, ctrl0, sigma, limits, W, seed=SEED, max_batch=B, arc_all=arc_all)
    job.set_shape(nt, g1)
    if order is not None:
        job.set_option(S.OPT_ORDER, order)
    r = run_sspp(job, B, first=first)
    ctrl_o, arc_o, feas_o = oracle_sample_score(b, knots, ctrl0, sigma, limits, first, B, arc_all)
    assert_sspp_parity(r, ctrl_o, arc_o, feas_o, first)
    return job, r, knots, ctrl0, ctrl_o, arc_o, feas_o


def steps_case(b, start, end, sigma, limits, steps, split):
    """A multi-step SsppSteps launch (steps x B candidates, the throughput shape), twice back to
    back: every step's feasibility, arcs and argmin record against the oracle."""
    import sspp_amd as S
    import torch
    knots, ctrl0 = linear_init(start, end, N_CTRL)
    first = 5 * B
    job = S.SsppJob(b.scene, knots, 3, ctrl0, sigma, limits, W, seed=SEED, max_batch=B)
    arcs = [torch.empty(steps * B, dtype=torch.float64, device="cuda")]
    feas = [torch.empty(steps * B, dtype=torch.uint8, device="cuda")]
    ex = S.SsppSteps([job], [torch.cuda.current_stream()], B, arcs, feas, steps_per_launch=steps)
    best = torch.zeros((steps, 4), dtype=torch.int64, device="cuda")
    for rep in range(2):
        ex.enqueue(steps, first + rep * steps * B, B, best)
        torch.cuda.synchronize()
        assert job.config()["shape"] == "128x4"
        assert job.get_option(S._lib.OPT_LAST_SPLIT) == split
        arc, fe, got = arcs[0].cpu().numpy(), feas[0].cpu().numpy(), best.cpu()
        for i in range(steps):
            f0 = first + (rep * steps + i) * B
            _, arc_o, feas_o = oracle_sample_score(b, knots, ctrl0, sigma, limits, f0, B)
            np.testing.assert_array_equal(fe[i * B:(i + 1) * B], feas_o)
            assert arc_err(arc[i * B:(i + 1) * B], arc_o) <= COST_TOL
            k, best_o = O.argmin(arc_o, feas_o)
            cost, idx, cnt = S.decode_best(got[i])
            assert idx == (f0 + k if k >= 0 else -1) and cnt == int(feas_o.sum()), (rep, i)
            if k >= 0:
                assert abs(cost - best_o) <= COST_TOL
    assert job.get_option(S._lib.OPT_SPLIT_LOST) == 0
    return job, knots, ctrl0


# ------------------------------------------------------------------ 1. the primitive zoo
def zoo_bundle(bundles, dof=7):
    return bundles("zoo", Y.zoo, 0, dof)


@pytest.mark.parametrize("arc_all", [False, True])
@pytest.mark.parametrize("nt,g1", LAUNCH)
def test_zoo_sample_score_matches_oracle(bundles, nt, g1, arc_all):
    """Plane (tilted, offset), sphere, tilted cylinder and rotated box statics against a mover of
    a box, an offset sphere and a tilted cylinder with a margin: 11 pairs, every supported pair
    type but mover-mover sphere-sphere; the cylinder-cylinder pair is filtered by its bits."""
    b = zoo_bundle(bundles)
    assert len(Y.moving_pairs(b.ref, 7)) == 11 == b.scene.info()["n_pairs"]
    job, r, knots, _, ctrl_o, arc_o, feas_o = sample_case(b, Y.ZOO_START, Y.ZOO_END, 0.2, Y.ZOO_LIMITS, nt, g1,
                                                           arc_all=arc_all)
    assert_mixed(b, knots, ctrl_o, feas_o, (Y.PLANE, Y.SPHERE, Y.CYLINDER, Y.BOX))
    cfg = job.config()
    assert cfg["sampled_pairs"] == 11 and cfg["cylinder_box"] and not cfg["split"]
    assert cfg["scan"] == Y.expected_scan(b.ref, 7) == "fp32-filtered"
    assert np.isinf(r["arc"]).sum() == (0 if arc_all else int((feas_o == 0).sum()))


@pytest.mark.parametrize("nt,g1", LAUNCH)
def test_zoo_score_ctrl_matches_oracle(bundles, nt, g1):
    """Caller-supplied control points on the zoo, end points perturbed too (no control point is
    the initial spline's: the full pair table, positions and quaternions everywhere)."""
    import sspp_amd as S
    import torch
    b = zoo_bundle(bundles)
    knots, ctrl0 = linear_init(Y.ZOO_START, Y.ZOO_END, N_CTRL)
    # the sampler's candidates (which meet the condition), every control point moved a little more
    ctrl = O.sample_sspp(ctrl0, 3, 0.2, Y.ZOO_LIMITS, SEED, 0, B) + \
        np.random.default_rng(SEED).normal(0, 0.03, size=(B, N_CTRL, 7)) * Y.ZOO_LIMITS
    job = S.SsppJob(b.scene, knots, 3, ctrl0, 0.2, Y.ZOO_LIMITS, W, seed=SEED, max_batch=B)
    job.set_shape(nt, g1)
    out = job.alloc(B)
    job.score_ctrl(torch.from_numpy(ctrl).cuda(), 0, out["arc"], out["feasible"], out["best"])
    torch.cuda.synchronize()
    key = ("score_ctrl",)
    if key not in b.memo:
        b.memo[key] = O.sspp_score(b.oscene, knots, 3, ctrl, W)
    arc_o, feas_o = b.memo[key]
    assert_mixed(b, knots, ctrl, feas_o, (Y.PLANE, Y.SPHERE, Y.CYLINDER, Y.BOX))
    np.testing.assert_array_equal(_np(out["feasible"]), feas_o)
    assert arc_err(_np(out["arc"]), arc_o) <= COST_TOL
    cost, idx, cnt = S.decode_best(out["best"])
    idx_o, best_o = O.argmin(arc_o, feas_o)
    assert idx == idx_o >= 0 and cnt == int(feas_o.sum()) and abs(cost - best_o) <= COST_TOL
    assert job.config()["scan"] == "fp32-filtered"


@pytest.mark.parametrize("nt,g1", LAUNCH)
def test_tilted_plane_hull_cull(bundles, nt, g1):
    """The plane branch of pair_may_touch on the device: k_sspp_c2f computes the survivors' hull
    masks only for tables of 9 to 64 pairs, so this scene has 12, and its job spreads the
    candidates widely along y (limit 3), the axis the plane's normal leans along.  Condition,
    from the oracle and the scene's numbers alone: for at least MIN_EACH candidates the plane is
    the only contact and the cull would drop it if it took the other end of the control points'
    y range (n . corner - slack >= 0 there) — a wrong selection frees them."""
    b = bundles("hull_cull", Y.hull_cull)
    job, r, knots, _, ctrl_o, arc_o, feas_o = sample_case(b, Y.ONE_START, Y.ONE_END, 0.2, Y.HULL_LIMITS, nt, g1)
    assert_mixed(b, knots, ctrl_o, feas_o, (Y.PLANE, Y.SPHERE))
    assert job.config()["sampled_pairs"] == 12 == b.scene.info()["n_pairs"]
    ref = b.ref
    plane = b.named("ramp")[0]
    qw, qx = np.array(Y.RAMP_QUAT[:2]) / np.linalg.norm(Y.RAMP_QUAT)
    normal = np.array([0.0, -2 * qw * qx, qw * qw - qx * qx])  # the plane's z axis (rotation about x)
    assert normal[1] < -0.1
    slack = max(float(np.linalg.norm(ref["geom_pos"][g])) + Y._rbound(ref["geom_type"][g], ref["geom_size"][g])
                for g in b.named("m_"))
    lo = ctrl_o[:, :, :3].min(axis=1)
    wrong_end = normal[1] * lo[:, 1] + normal[2] * lo[:, 2] - normal @ ref["geom_pos"][plane]
    only_plane = (feas_o == 0) & (oracle_feasible(b, knots, ctrl_o, skip_types=(Y.PLANE,)) == 1)
    assert int((only_plane & (wrong_end - slack >= 0)).sum()) >= MIN_EACH


# ------------------------------------------------------------------ 2. one-type scenes
ONE_SIGMA = 0.12
ONE_TYPES = {"spheres": Y.SPHERE, "boxes": Y.BOX, "cylinders": Y.CYLINDER}


@pytest.mark.parametrize("nt,g1", LAUNCH)
@pytest.mark.parametrize("kind", ["spheres", "boxes", "cylinders"])
def test_one_type_single_launch(bundles, kind, nt, g1):
    """A single-geom box mover over the tilted plane and statics of one kind: the FP32-filtered
    scan on a table the filter must send to the FP64 lane entirely (spheres, cylinders: pair
    types it does not handle) or decides itself (boxes), with the tilted plane in both."""
    b = bundles(kind, lambda: Y.one_type(kind))
    job, r, knots, _, ctrl_o, arc_o, feas_o = sample_case(b, Y.ONE_START, Y.ONE_END, ONE_SIGMA, Y.ZOO_LIMITS, nt, g1)
    assert_mixed(b, knots, ctrl_o, feas_o, (Y.PLANE, ONE_TYPES[kind]))
    cfg = job.config()
    assert cfg["scan"] == Y.expected_scan(b.ref, 7) == "fp32-filtered"
    assert cfg["sampled_pairs"] == len(Y.moving_pairs(b.ref, 7))
    assert cfg["cylinder_box"] == (kind == "cylinders") and not cfg["split"]


@pytest.mark.parametrize("kind", ["spheres", "boxes"])
def test_one_type_split_launch(bundles, kind):
    """8 steps x 2048 candidates in one launch: single moving geom, no cylinder-box pair, one
    mover, so the launch runs split (the survivor queue), and surv_finish finishes survivors
    whose deciding pair is a sphere or the tilted plane.  Every step equals the oracle and no
    survivor is lost."""
    b = bundles(kind, lambda: Y.one_type(kind))
    job, knots, ctrl0 = steps_case(b, Y.ONE_START, Y.ONE_END, ONE_SIGMA, Y.ZOO_LIMITS, 8, split=1)
    ctrl_o, _, feas_o = oracle_sample_score(b, knots, ctrl0, ONE_SIGMA, Y.ZOO_LIMITS, 5 * B, B)
    assert_mixed(b, knots, ctrl_o, feas_o, (Y.PLANE, ONE_TYPES[kind]))
    assert not job.config()["cylinder_box"]


def test_cylinder_scene_does_not_split(bundles):
    """The same launch over one vertical and one tilted static cylinder: a cylinder-box table
    never splits (the settle step decides those pairs), and every step equals the oracle."""
    b = bundles("cylinders", lambda: Y.one_type("cylinders"))
    job, knots, ctrl0 = steps_case(b, Y.ONE_START, Y.ONE_END, ONE_SIGMA, Y.ZOO_LIMITS, 8, split=0)
    ctrl_o, _, feas_o = oracle_sample_score(b, knots, ctrl0, ONE_SIGMA, Y.ZOO_LIMITS, 5 * B, B)
    assert_mixed(b, knots, ctrl_o, feas_o, (Y.PLANE, Y.CYLINDER))
    assert job.config()["cylinder_box"]


# ------------------------------------------------------------------ 3. the pair-count boundary
GRIDS = [(4, 16), (5, 13), (3, 24)]
GRID_SIGMA = 0.06


def grid_last_pairs(b, nm, ns):
    """The geoms of the last pairs of the scene-order table (pairs grouped by moving geom, the
    statics in scene order within a group): index >= 64, or the 64th pair itself (index 63, the
    mask word's top bit) in the 64-pair table."""
    first_static = (64 if nm * ns > 64 else 63) - (nm - 1) * ns
    return b.named("st")[first_static:], b.named("mv")[-1:]


@pytest.mark.parametrize("order", ["scene", "default"])
@pytest.mark.parametrize("nt,g1", LAUNCH)
@pytest.mark.parametrize("nm,ns", GRIDS)
def test_pair_count_boundary(bundles, nm, ns, nt, g1, order):
    """64, 65 and 72 pairs: past 64 the candidate hull mask is all ones, the FP32 filter is off,
    the hit-order pre-pass leaves the gap order and the <= 64-pair kernel forms are skipped.

    The kernels index the job's table, not the scene's: a sampled job sorts its pairs by their
    gap to the mean path, which moves this scene's deciding pair to the front.  So each grid
    runs twice.  "scene": SSPP_OPT_ORDER 0 keeps the scene order (asserted), and the condition
    then speaks about the table the device walks: for at least MIN_EACH candidates every contact
    is a pair of table index >= 64 (index 63 in the 64-pair table) — they are free without the
    last statics and free without the last moving geom — so a scan that dropped or mis-masked the
    entries from 64 on would call them feasible.  "default": the library's order, parity only."""
    import sspp_amd as S
    b = bundles("grid_%dx%d" % (nm, ns), lambda: Y.grid(nm, ns))
    job, r, knots, _, ctrl_o, arc_o, feas_o = sample_case(b, Y.GRID_START, Y.GRID_END, GRID_SIGMA, Y.ZOO_LIMITS, nt, g1,
                                                           order=0 if order == "scene" else None)
    assert job.get_option(S._lib.OPT_NPAIRS) == nm * ns == b.scene.info()["n_pairs"]
    assert job.config()["scan"] == Y.expected_scan(b.ref, 7) == ("fp32-filtered" if nm * ns <= 64 else "fp64")
    assert_mixed(b, knots, ctrl_o, feas_o, ())
    if order == "scene":
        assert job.config()["pair_order"] == "scene"
        # the scene order of the pairs, as the condition indexes them: moving geom major
        pairs = sorted(Y.moving_pairs(b.ref, 7))
        statics, movers = grid_last_pairs(b, nm, ns)
        first = 64 if nm * ns > 64 else 63
        assert pairs[first:] == [(movers[0], g) for g in statics]
        only_last = (feas_o == 0) & (oracle_feasible(b, knots, ctrl_o, off=statics) == 1) & \
            (oracle_feasible(b, knots, ctrl_o, off=movers) == 1)
        assert int(only_last.sum()) >= MIN_EACH


@pytest.mark.parametrize("nt,g1", [(0, 0), (128, 4)])
def test_fp32_filter_is_invisible_at_64_pairs(bundles, nt, g1):
    """The largest table the FP32 filter takes: SSPP_OPT_F32 off against on, bit-identical."""
    import sspp_amd as S
    b = bundles("grid_4x16", lambda: Y.grid(4, 16))
    knots, ctrl0 = linear_init(Y.GRID_START, Y.GRID_END, N_CTRL)
    res = {}
    for f32 in (1, 0):
        job = S.SsppJob(b.scene, knots, 3, ctrl0, GRID_SIGMA, Y.ZOO_LIMITS, W, seed=SEED, max_batch=B)
        job.set_shape(nt, g1)
        job.set_option(S.OPT_F32, f32)
        res[f32] = run_sspp(job, B, first=3 * B)
        assert job.get_option(S._lib.OPT_LAST_F32) == f32
    for k in ("ctrl", "feasible", "arc"):
        np.testing.assert_array_equal(res[1][k], res[0][k], err_msg=k)
    assert res[1]["best"] == res[0]["best"]
    assert MIN_EACH <= int(res[1]["feasible"].sum()) <= B - MIN_EACH


# ------------------------------------------------------------------ 4. the filter's certified range
# offset along x -> the scan: the scene's farthest static sits 0.4 m past the offset, and f32_eps
# turns the filter off when a static is more than 16 m from the origin along an axis
OFFSETS = {0.0: "fp32-filtered", 7.5: "fp32-filtered", 8.5: "fp32-filtered", 15.5: "fp32-filtered", 16.5: "fp64"}
MIRRORED = 15.5  # this offset also carries a copy of the statics far along -y (within 16 m)


def shifted_bundle(bundles, dx):
    return bundles("boxes_x%g" % dx, lambda: Y.one_type("boxes", (dx, 0.0, 0.0), mirror=(dx == MIRRORED)))


@pytest.mark.parametrize("nt,g1", LAUNCH)
@pytest.mark.parametrize("dx", list(OFFSETS))
def test_filter_range_offsets(bundles, dx, nt, g1):
    """The boxes scene and its path translated along x: beyond 8 m the kernel sends positions to
    the FP64 lane, beyond 16 m f32_eps turns the filter off.  Each offset against the oracle at
    that offset (translation changes rounding).  The mirrored copy at 15.5 m is out of the
    sampled candidates' reach: the sampled table drops it, caller splines scan it."""
    import sspp_amd as S
    import torch
    b = shifted_bundle(bundles, dx)
    sh = np.array([dx, 0, 0, 0, 0, 0, 0.0])
    job, r, knots, ctrl0, ctrl_o, arc_o, feas_o = sample_case(b, Y.ONE_START + sh, Y.ONE_END + sh, ONE_SIGMA,
                                                               Y.ZOO_LIMITS, nt, g1)
    assert_mixed(b, knots, ctrl_o, feas_o, (Y.PLANE, Y.BOX))
    far = float(np.abs(b.ref["geom_pos"]).max())
    assert (far > 16.0) == (OFFSETS[dx] == "fp64")
    assert job.config()["scan"] == Y.expected_scan(b.ref, 7) == OFFSETS[dx]
    assert job.config()["sampled_pairs"] == 4
    if dx == MIRRORED:
        assert b.scene.info()["n_pairs"] == 7 and np.abs(b.ref["geom_pos"]).max() > 15.5
        out = job.alloc(B)
        job.score_ctrl(torch.from_numpy(ctrl_o.copy()).cuda(), 0, out["arc"], out["feasible"], out["best"])
        torch.cuda.synchronize()
        assert job.config()["scan"] == "fp32-filtered"
        np.testing.assert_array_equal(_np(out["feasible"]), feas_o)
        assert arc_err(_np(out["arc"]), arc_o) <= COST_TOL
        cost, idx, cnt = S.decode_best(out["best"])
        idx_o, best_o = O.argmin(arc_o, feas_o)
        assert idx == idx_o >= 0 and cnt == int(feas_o.sum()) and abs(cost - best_o) <= COST_TOL


@pytest.mark.parametrize("nt,g1", LAUNCH)
def test_filter_extent_edge(bundles, nt, g1):
    """A static box whose bounding radius passes 8 m (a 12 m table under the boxes): the pair's
    extent leaves the filter's certified range and the whole table is scanned in FP64."""
    b = bundles("big_table", Y.big_table)
    job, r, knots, _, ctrl_o, arc_o, feas_o = sample_case(b, Y.ONE_START, Y.ONE_END, ONE_SIGMA, Y.ZOO_LIMITS, nt, g1)
    assert_mixed(b, knots, ctrl_o, feas_o, (Y.BOX,))
    table = b.named("table")
    assert int(oracle_feasible(b, knots, ctrl_o, off=table).sum()) > int(feas_o.sum())  # the table decides some
    assert job.config()["scan"] == Y.expected_scan(b.ref, 7) == "fp64"
    assert job.config()["sampled_pairs"] == 5


# ------------------------------------------------------------------ 5. two movers, cut windows
TWO_LIMITS = np.array([1, 1, 1, .3, .3, .3, .3, 1, 1])


@pytest.mark.parametrize("nt,g1", LAUNCH)
def test_two_movers_match_oracle(bundles, nt, g1):
    """D = 9: body 0 moves fully, body 1 in x and y only (its z and rotation stay at qpos0).
    Per-candidate parity; condition: some candidates' only contacts are mover-mover pairs (free
    without body 1's geoms and free without the statics)."""
    b = bundles("two_movers", Y.two_movers, 0, 9)
    assert b.scene.info()["n_movers"] == 2 and b.scene.info()["n_pairs"] == 12
    job, r, knots, _, ctrl_o, arc_o, feas_o = sample_case(b, Y.TWO_START, Y.TWO_END, 0.15, TWO_LIMITS, nt, g1)
    assert_mixed(b, knots, ctrl_o, feas_o, (Y.SPHERE, Y.BOX))
    only_mm = (feas_o == 0) & (oracle_feasible(b, knots, ctrl_o, off=b.named("b_")) == 1) & \
        (oracle_feasible(b, knots, ctrl_o, off=b.named("ball") + b.named("slab")) == 1)
    assert int(only_mm.sum()) >= MIN_EACH
    cfg = job.config()
    assert cfg["sampled_pairs"] == 12 and not cfg["split"] and cfg["scan"] == Y.expected_scan(b.ref, 9)


@pytest.mark.parametrize("nt,g1", LAUNCH)
def test_zoo_cut_quaternion_window(bundles, nt, g1):
    """D = 6 on the zoo: the window ends inside the quaternion (w, x from the spline, y, z from
    qpos0), which is then normalised."""
    b = zoo_bundle(bundles, 6)
    job, r, knots, _, ctrl_o, arc_o, feas_o = sample_case(b, Y.ZOO_START[:6], Y.ZOO_END[:6], 0.2, Y.ZOO_LIMITS[:6],
                                                           nt, g1)
    assert_mixed(b, knots, ctrl_o, feas_o, (Y.PLANE, Y.SPHERE, Y.CYLINDER, Y.BOX))
    assert job.config()["sampled_pairs"] == 11 and job.config()["cylinder_box"]


# ------------------------------------------------------------------ 6. TaskSpacePlanner
TSP_B, TSP_CP = 1024, 64
# scene -> (xml, the geoms whose deep contacts the case is about, the form the library picks for
# 1024 candidates: the deferred box-box polygons (3) need a box-box pair, else the inline k_tsp)
TSP_SCENES = {"boxes": (Y.tsp_boxes, ("ball", "tilt"), 3),
              "cylinders_vertical": (lambda: Y.tsp_cylinders(False), ("c0", "c1", "c2"), 0),
              "cylinders_tilted": (lambda: Y.tsp_cylinders(True), ("c1",), 0)}


@pytest.mark.parametrize("form", [-1, 0])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", list(TSP_SCENES))
def test_tsp_synthetic_matches_oracle(bundles, name, K, form):
    """k_tsp where the scene, not an option, picks the narrowphase: a non-upright static box with
    a yaw-only mover (generic box-box), a sphere in the cost, an all-vertical cylinder table
    (cb_upright_sd only) and one with a tilted cylinder (the candidate search).

    The library reports only the form that ran (SSPP_OPT_TSP_FORM); it does not report the
    upright / cylinder-box template a scene selects, so that the two cylinder scenes take different
    cylinder-box code is known from the host's choice (kscene: cbup) and not asserted here.  With
    no box-box pair the library's own choice for them is form 0, so their -1 and 0 runs are the
    same kernel."""
    import sspp_amd as S
    import torch
    xml, targets, picked = TSP_SCENES[name]
    b = bundles("tsp_" + name, xml, 1, "mover")
    mean = np.array([Y.TSP_START + (Y.TSP_END - Y.TSP_START) * (i + 1) / (K + 1) for i in range(K)])
    sigma = np.full((K, 4), 0.15)
    job = S.TspJob(b.scene, Y.TSP_START, Y.TSP_END, K, TSP_CP, mean=mean, sigma=sigma, lo=Y.TSP_LO, hi=Y.TSP_HI,
                   z_min=0.0, seed=SEED, max_batch=TSP_B)
    job.set_option(S.OPT_TSP_FORM, form)
    out = job.alloc(TSP_B, with_vias=True)
    job.sample_score(5, TSP_B, out["L"], out["Cnf"], out["Cwf"], out["status"], out["cost"], out["best"],
                     vias_out=out["vias"])
    torch.cuda.synchronize()
    assert job.get_option(S.OPT_TSP_FORM) == (picked if form < 0 else 0)
    vias = _np(out["vias"])
    if ("tsp", K) not in b.memo:
        vias_o = O.sample_tsp(mean, sigma, Y.TSP_LO, Y.TSP_HI, 0.0, SEED, 5, TSP_B)
        b.memo["tsp", K] = (vias_o, O.tsp_score(b.oscene, Y.TSP_START, Y.TSP_END, vias_o, TSP_CP))
    vias_o, (L, Cnf, Cwf, st, cost) = b.memo["tsp", K]
    # condition (the oracle's own via sets): both statuses, and each target geom in deep contact
    # for some candidates (their C_nf / C_wf is non-zero and changes without that geom)
    assert MIN_EACH <= int(st.sum()) <= TSP_B - MIN_EACH
    for t in targets:
        if ("tsp_off", K, t) not in b.memo:
            b.memo["tsp_off", K, t] = O.tsp_score(b.reduced(off=b.named(t)), Y.TSP_START, Y.TSP_END, vias_o, TSP_CP)
        _, Cnf2, Cwf2, _, _ = b.memo["tsp_off", K, t]
        deep = ((Cnf != 0) | (Cwf != 0)) & ((Cnf2 != Cnf) | (Cwf2 != Cwf))
        assert int(deep.sum()) >= MIN_EACH, t
    assert np.abs(vias - vias_o).max() <= 1e-12
    if not np.array_equal(vias, vias_o):  # score the via sets the GPU scored
        L, Cnf, Cwf, st, cost = O.tsp_score(b.oscene, Y.TSP_START, Y.TSP_END, vias, TSP_CP)
    np.testing.assert_array_equal(_np(out["status"]), st)
    for a, o in ((out["L"], L), (out["Cnf"], Cnf), (out["Cwf"], Cwf), (out["cost"], cost)):
        assert np.abs(_np(a) - o).max() <= 1e-9
    idx_o, _ = O.tsp_best(cost, st)
    c, idx, cnt = S.decode_best(out["best"])
    assert cnt == int(st.sum())
    assert idx == (idx_o + 5 if idx_o >= 0 else -1)
