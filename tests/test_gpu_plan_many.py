"""Query launches at the job level: sspp_job_set_queries + sspp_job_sample_score_queries.

Step q of a query launch is query q: its own initial spline, sigma, limits and seed.  Every case
compares three ways:
  (A) the query launch;
  (B) the same job re-targeted to each query (SsppJob.update) and run with the ordinary single
      launch — the path the existing parity tests pin;
  (C) the CPU oracle on the oracle's own samples (capsule scene: its composed numpy reference).
A against B is byte-equal (arc, feasible, ctrl_out, the best record); A against C holds the
project's bars: control points bit-equal, feasibility identical, arcs within COST_TOL.

The queries are chosen on the CPU with the oracle, and every case with collisions asserts from the
oracle alone that at least one query has 0 < count < B.

The sampled rows of a degree-p spline are [p, n - p): a cubic needs n >= 7 control points to have
one (n = 6 has none, as n = 4: every candidate is then the initial spline and a query's count is 0
or B).  The cases that are about per-query sampling therefore use n = 7; n = 4 and n = 6 are the
degenerate sets, whose non-emptiness condition is one query with count 0 and one with count B.
"""
import os

import numpy as np
import pytest

from oracle import mjcf_ref
from oracle import oracle as O
from tests import capsule_scenes as CS
from tests import dof_degree_cases as DD
from tests import synth_scenes as Y
from tests.conftest import SCENES, arc_err
from tests.test_gpu_parity import COST_TOL, _np

pytestmark = pytest.mark.gpu

ROBOCRANE = os.path.join(SCENES, "robocrane.xml")
QUAT = np.array([0.707, 0.0, 0.0, 0.707])
E_INVAL = r"\(-1\)"


def pose(x, y, z):
    return np.concatenate([[x, y, z], QUAT])


class Query:
    def __init__(self, start, end, sigma, limits, seed, n, p=3):
        u = np.array([i / (n - 1) for i in range(n)])
        self.knots, self.ctrl0 = O.interpolate(np.array([(1 - t) * start + t * end for t in u]), p, u)
        self.sigma, self.limits, self.seed, self.p = float(sigma), np.asarray(limits, np.float64), int(seed), p


# robocrane queries (oracle counts of 70 candidates, W = 16, n = 7, ids from 0: 12, 33, 47, 0, 70)
def crane_queries(n=7):
    return [Query(pose(0.5, 0.15, 0.19), pose(0.5, -0.05, 0.19), 0.1, np.ones(7), 1, n),
            Query(pose(0.5, 0.15, 0.2), pose(0.5, -0.05, 0.2), 0.1, np.ones(7), 2, n),
            Query(pose(0.45, 0.2, 0.22), pose(0.55, -0.1, 0.22), 0.12, [.5, 1, 1, .2, .2, .2, .2], 4, n)]


def floor_query(n=7):   # the straight line lies in the floor
    return Query(pose(0.3, 0.2, 0.01), pose(0.5, 0.2, 0.01), 0.001, np.ones(7), 5, n)


def hover_query(n=7):   # far above everything
    return Query(pose(0.3, 0.2, 0.5), pose(0.5, 0.2, 0.5), 0.01, np.ones(7), 6, n)


@pytest.fixture(scope="module")
def crane(cuda):
    import sspp_amd as S
    return S.Scene(S.Model(ROBOCRANE), 0, 7), O.Scene(mjcf_ref.load(ROBOCRANE), 0, 7)


def make_job(scene, q, W, B, **kw):
    import sspp_amd as S
    return S.SsppJob(scene, q.knots, q.p, q.ctrl0, q.sigma, q.limits, W, seed=q.seed, max_batch=B, **kw)


def set_queries(job, qs):
    job.set_queries(np.stack([q.ctrl0 for q in qs]), [q.sigma for q in qs], np.stack([q.limits for q in qs]),
                    [q.seed for q in qs])


def run_set(job, qs, B, first=0, with_ctrl=True):
    """(A): one query launch; numpy outputs, best as int64 [Q, 4] records."""
    import torch
    set_queries(job, qs)
    out = job.alloc_queries(len(qs), B, with_ctrl=with_ctrl)
    job.sample_score_queries(first, B, out["arc"], out["feasible"], out["best"], ctrl_out=out.get("ctrl"))
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def run_single(job, q, B, first=0, with_ctrl=True):
    """(B): the job re-targeted to q, one ordinary launch."""
    import torch
    job.update(q.ctrl0, q.sigma, q.limits, q.seed)
    out = job.alloc(B, with_ctrl=with_ctrl)
    job.sample_score(first, B, out["arc"], out["feasible"], out["best"], ctrl_out=out.get("ctrl"))
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def oracle_scorer(oscene, W):
    def score(q, ctrl):
        arc, feas = O.sspp_score(oscene, q.knots, q.p, ctrl, W)
        return arc, feas, np.ones(len(arc), bool)
    return score


def assert_query_equal(a, b, q, what):
    for k in b:
        got = a[k][q]
        assert got.tobytes() == np.ascontiguousarray(b[k]).reshape(got.shape).tobytes(), (what, k, q)


def check_set(job, qs, B, score, first=0, with_ctrl=True, need_mixed=True):
    """A against B (bytes) and against C (the project's bars) for every query; returns the oracle's counts."""
    import sspp_amd as S
    a = run_set(job, qs, B, first, with_ctrl)
    assert job.get_option(S._lib.OPT_LAST_QUERIES) == len(qs)
    assert job.get_option(S._lib.OPT_LAST_SPLIT) == 0
    recs = S.check_records(a["best"])
    counts = []
    for i, q in enumerate(qs):
        b = run_single(job, q, B, first, with_ctrl)
        assert job.get_option(S._lib.OPT_LAST_QUERIES) == 0
        assert_query_equal(a, b, i, "query launch against the re-targeted job")
        ctrl_o = O.sample_sspp(q.ctrl0, q.p, q.sigma, q.limits, q.seed, first, B)
        if with_ctrl:
            assert np.array_equal(a["ctrl"][i], ctrl_o), i
        arc_o, feas_o, keep = score(q, ctrl_o)
        np.testing.assert_array_equal(a["feasible"][i][keep], feas_o[keep])
        assert arc_err(a["arc"][i][keep], arc_o[keep]) <= COST_TOL
        counts.append(int(feas_o.sum()))
        if keep.all():
            idx_o, best_o = O.argmin(arc_o, feas_o)
            cost, idx, cnt = S.decode_best(recs[i])
            assert cnt == counts[-1] and idx == (idx_o + first if idx_o >= 0 else -1), i
            assert (cost == np.inf) if idx_o < 0 else (abs(cost - best_o) <= COST_TOL)
    if need_mixed:
        assert any(0 < c < B for c in counts), counts
    return a, counts


# ------------------------------------------------------------------ distinct queries
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("nt,g1", [(256, 64), (128, 4), (256, 16)])
def test_distinct_queries(crane, nt, g1, f32, order):
    """Three queries that differ in start, end, sigma, limits and seed; B = 70 ends every step in a
    partial workgroup (4, 32 and 16 candidates per workgroup): a wrong step offset into the
    initial splines, limits, sigmas, seeds, the FP32 copies of the fixed rows or ctrl_out shows."""
    import sspp_amd as S
    scene, oscene = crane
    qs = crane_queries()
    job = make_job(scene, qs[0], 16, 70)
    job.set_shape(nt, g1)
    job.set_option(S.OPT_F32, f32)
    job.set_option(S.OPT_ORDER, order)
    _, counts = check_set(job, qs, 70, oracle_scorer(oscene, 16), first=2 ** 33 - 30)
    assert (job.get_option(S._lib.OPT_LAST_NT), job.get_option(S._lib.OPT_LAST_G1)) == (nt, g1)
    assert len(set(counts)) == 3, counts   # by the oracle the three queries do differ


def test_isolation(crane):
    """Nothing feasible, everything feasible, mixed: an argmin record or an arrival counter that
    leaked between steps would show in the records."""
    import sspp_amd as S
    scene, oscene = crane
    qs = [floor_query(), hover_query(), crane_queries()[1]]
    B = 70
    job = make_job(scene, qs[0], 16, B)
    a, counts = check_set(job, qs, B, oracle_scorer(oscene, 16))
    recs = [S.decode_best(r) for r in S.check_records(a["best"])]
    assert counts[0] == 0 and recs[0] == (np.inf, -1, 0)
    assert counts[1] == B and recs[1][2] == B
    assert 0 < counts[2] < B and recs[2][2] == counts[2]
    arc2, feas2 = a["arc"][2], a["feasible"][2]
    assert recs[2][1] == O.argmin(arc2, feas2)[0] and recs[2][0] == arc2[recs[2][1]]


def test_degenerate_queries(crane):
    """sigma = 0 (every candidate is the initial spline), start = end (a spline of one point:
    arc length 0 for the unperturbed part), beside a mixed query."""
    scene, oscene = crane
    here = pose(0.5, 0.05, 0.25)
    qs = [Query(pose(0.5, 0.15, 0.3), pose(0.5, -0.05, 0.3), 0.0, np.ones(7), 8, 7),
          Query(here, here, 0.1, np.ones(7), 7, 7),
          Query(pose(0.5, 0.15, 0.136), pose(0.5, -0.05, 0.136), 0.0, np.ones(7), 9, 7),
          crane_queries()[1]]
    job = make_job(scene, qs[0], 16, 70)
    a, counts = check_set(job, qs, 70, oracle_scorer(oscene, 16))
    assert counts[0] == 70 and counts[2] == 0 and 0 < counts[1] < 70
    assert len(set(a["arc"][0].tolist())) == 1   # sigma = 0: one spline, 70 times


@pytest.mark.parametrize("n", [4, 6])
def test_no_sampled_rows(crane, n):
    """init_points 4 and 6: a cubic has no sampled row (nrd = 0), every candidate of a query is
    its initial spline, so a query's count is 0 or B — one of each here."""
    scene, oscene = crane
    qs = [floor_query(n), hover_query(n), Query(pose(0.5, 0.15, 0.136), pose(0.5, -0.05, 0.136), 0.1, np.ones(7), 3, n)]
    job = make_job(scene, qs[0], 16, 70)
    _, counts = check_set(job, qs, 70, oracle_scorer(oscene, 16), need_mixed=False)
    assert counts == [0, 70, 0]


# ------------------------------------------------------------------ the pair table of a set
def far_apart():
    """Two boxes 10 m apart and a box mover: a query near one cannot reach the other."""
    statics = [Y.geom(Y.BOX, (0.05, 0.05, 0.05), (0.25, 0.0, 0.3), name="near"),
               Y.geom(Y.BOX, (0.05, 0.05, 0.05), (10.25, 0.0, 0.3), name="far")]
    return Y.mjcf(statics, [Y.body("mover", (0, 0, 0.3), [Y.geom(Y.BOX, Y.MOVER_BOX, name="m_box")])])


@pytest.fixture(scope="module")
def scratch(tmp_path_factory):
    return str(tmp_path_factory.mktemp("plan_many_scenes"))


def load_scene(root, name, text, D):
    import sspp_amd as S
    path = os.path.join(root, name + ".xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(text)
    return S.Scene(S.Model(path), 0, D), O.Scene(mjcf_ref.load(path), 0, D)


@pytest.mark.parametrize("swap", [False, True])
def test_pair_table_of_a_set(cuda, scratch, swap):
    import sspp_amd as S
    scene, oscene = load_scene(scratch, "far_apart", far_apart(), 7)
    assert scene.info()["n_pairs"] == 2

    def q(x0, seed):
        return Query(np.array([x0, 0, 0.38, 1, 0, 0, 0.]), np.array([x0 + 0.5, 0, 0.38, 1, 0, 0, 0.]), 0.1,
                     Y.ZOO_LIMITS, seed, 7)
    qs = [q(0.0, 5), q(10.0, 6)]
    if swap:
        qs.reverse()
    job = make_job(scene, qs[0], 16, 40)
    # each obstacle is missing from the other query's own table ...
    assert job.get_option(S._lib.OPT_NPAIRS) == 1
    job.update(qs[1].ctrl0, qs[1].sigma, qs[1].limits, qs[1].seed)
    assert job.get_option(S._lib.OPT_NPAIRS) == 1
    # ... and both are in the set's; each query collides with its own
    set_queries(job, qs)
    assert job.get_option(S._lib.OPT_NPAIRS) >= 2
    _, counts = check_set(job, qs, 40, oracle_scorer(oscene, 16))
    assert all(0 < c < 40 for c in counts), counts
    job.update(qs[0].ctrl0, qs[0].sigma, qs[0].limits, qs[0].seed)
    assert job.get_option(S._lib.OPT_NPAIRS) == 1   # the job's own table is its own again


# ------------------------------------------------------------------ kernel forms, dofs, degrees
def two_queries(D, p, n):
    """The (D, p) path of tests/dof_degree_cases.py and a second one beside it (other sigma,
    limits and seed)."""
    s, e, lim = DD.ends(D)
    out = []
    for k, (dy, sg, seed) in enumerate([(0.0, DD.sigma_for(D), 11), (0.03, DD.sigma_for(D) * 1.5, 12)]):
        s2, e2 = s.copy(), e.copy()
        if D >= 2:
            s2[1] += dy
            e2[1] -= dy
        else:
            s2[0] += dy
        out.append(Query(s2, e2, sg, lim * (1.0 if k == 0 else 0.8), seed, n, p))
    return out


FORMS = {   # name: (scene text, D, p, n, (one geom, cylinder-box or capsule pairs))
    "two_geom_cbx": (DD.window, 7, 3, 7, (0, 1)),
    "one_geom_cbx": (DD.window_one, 7, 3, 7, (1, 1)),
    "two_geom": (lambda: DD._window(False, cylinder=False), 7, 3, 7, (0, 0)),
    "one_geom": (DD.window_one_nocyl, 7, 3, 7, (1, 0)),
    "two_movers_p3": (Y.two_movers, 9, 3, 7, None),
    "two_movers_p2": (Y.two_movers, 9, 2, 5, None),
    "dof3_p2": (DD.window, 3, 2, 5, None),
    "dof1_p3": (DD.window, 1, 3, 7, None),
}


@pytest.mark.parametrize("name", sorted(FORMS))
def test_kernel_forms(cuda, scratch, name):
    """Q = 2, B = 40 on every non-split form (one-geom or not, CBX or not, NM = 2 for dof 9) and
    on other dofs and degree 2, at the latency shape and the throughput shape."""
    import sspp_amd as S
    text, D, p, n, form = FORMS[name]
    scene, oscene = load_scene(scratch, name, text(), D)
    qs = two_queries(D, p, n)
    job = make_job(scene, qs[0], 16, 40)
    check_set(job, qs, 40, oracle_scorer(oscene, 16))
    assert job.get_option(S._lib.OPT_LAST_NT) == 256
    job.set_shape(128, 4)
    check_set(job, qs, 40, oracle_scorer(oscene, 16))
    if form is not None:
        set_queries(job, qs)
        assert job.get_option(S._lib.OPT_CYLBOX) == form[1]
        assert (scene.info()["n_moving_geoms"] == 1) == bool(form[0])
    if D == 9:
        assert scene.info()["n_movers"] == 2


def test_capsule_table(cuda, tmp_path_factory):
    """A capsule mover (the CBX form through capsule pairs) against the composed numpy reference."""
    import sspp_amd as S
    from tests.test_gpu_capsule import Bundle
    b = Bundle(str(tmp_path_factory.mktemp("plan_many_capsule")), "capsule_mover", CS.sspp_capsule_mover, 0, 7)
    qs = [Query(CS.START, CS.END, CS.SIGMA, CS.LIMITS, 7, 7),
          Query(CS.START + [0, 0.03, 0.02, 0, 0, 0, 0], CS.END + [0, -0.03, 0.02, 0, 0, 0, 0], 0.1, CS.LIMITS * 0.8, 8, 7)]

    def score(q, ctrl):
        r = CS.sspp_reference(b.ref, q.knots, ctrl, 16, 7)
        return r["arc"], r["feas"], ~r["near"]
    job = make_job(b.scene, qs[0], 16, 40)
    check_set(job, qs, 40, score)
    set_queries(job, qs)
    assert job.get_option(S._lib.OPT_CAPSULE) == 1


# ------------------------------------------------------------------ sizes
def many_queries(Q, n=7):
    return [Query(pose(0.5, 0.15 + 0.002 * k, 0.19 + 0.0005 * k), pose(0.5, -0.05, 0.2), 0.08 + 0.001 * k, np.ones(7),
                  100 + k, n) for k in range(Q)]


def test_one_query_equals_the_single_launch(crane):
    scene, oscene = crane
    qs = crane_queries()[1:2]
    job = make_job(scene, qs[0], 16, 70)
    check_set(job, qs, 70, oracle_scorer(oscene, 16))


def test_sixty_four_queries(crane):
    scene, oscene = crane
    qs = many_queries(64)
    job = make_job(scene, qs[0], 16, 8)
    a, counts = check_set(job, qs, 8, oracle_scorer(oscene, 16))
    assert a["arc"].shape == (64, 8)


def test_sixteen_thousand_candidates_do_not_split(crane):
    """4 x 4096 candidates: an ordinary multi-step launch of this size splits; a query launch
    takes the throughput shape and does not."""
    import sspp_amd as S
    scene, oscene = crane
    qs = crane_queries() + [hover_query()]
    job = make_job(scene, qs[0], 16, 4096)
    _, counts = check_set(job, qs, 4096, oracle_scorer(oscene, 16), with_ctrl=False)
    run_set(job, qs, 4096, with_ctrl=False)
    assert job.get_option(S._lib.OPT_LAST_SPLIT) == 0
    assert job.get_option(S._lib.OPT_LAST_NT) == 128 and job.get_option(S._lib.OPT_LAST_G1) == 4
    assert job.get_option(S._lib.OPT_LAST_QUERIES) == 4
    assert counts[3] == 4096 and all(0 < c < 4096 for c in counts[:3]), counts


def test_job_state_survives_a_query_launch(crane):
    """The job's own query is untouched by set_queries and by a query launch; a second set
    replaces the first."""
    scene, oscene = crane
    own = crane_queries()[2]
    job = make_job(scene, own, 16, 70)
    import torch

    def ordinary():
        out = job.alloc(70, with_ctrl=True)
        job.sample_score(3, 70, out["arc"], out["feasible"], out["best"], ctrl_out=out["ctrl"])
        torch.cuda.synchronize()
        return {k: _np(v).tobytes() for k, v in out.items()}
    before = ordinary()
    first = run_set(job, crane_queries()[:2], 70, first=3)
    assert ordinary() == before
    others = [floor_query(), crane_queries()[1], hover_query()]
    second = run_set(job, others, 70, first=3)
    assert ordinary() == before
    assert second["arc"].shape == (3, 70)
    assert second["arc"][1].tobytes() == first["arc"][1].tobytes()
    assert second["feasible"][0].sum() == 0 and second["feasible"][2].sum() == 70
    check_set(job, others, 70, oracle_scorer(oscene, 16), first=3)


# ------------------------------------------------------------------ refusals
def test_refusals(crane):
    import sspp_amd as S
    scene, _ = crane
    qs = crane_queries()
    job = make_job(scene, qs[0], 16, 70)
    out = job.alloc_queries(3, 70)
    with pytest.raises(S.SsppError, match=E_INVAL):      # no set yet
        job.sample_score_queries(0, 70, out["arc"], out["feasible"], out["best"])
    many = many_queries(65)
    with pytest.raises(S.SsppError, match=E_INVAL):
        set_queries(job, many)
    with pytest.raises(S.SsppError, match=E_INVAL):
        job.set_queries(np.zeros((0, 7, 7)), [], np.zeros((0, 7)), [])
    with pytest.raises(S.SsppError, match=E_INVAL):      # the refused sets left no set behind
        job.sample_score_queries(0, 70, out["arc"], out["feasible"], out["best"])
    with pytest.raises(ValueError):
        job.set_queries(np.zeros((3, 6, 7)), [0.1] * 3, np.ones((3, 7)), [1, 2, 3])
    with pytest.raises(ValueError):
        job.set_queries(np.zeros((3, 7, 7)), [0.1] * 2, np.ones((3, 7)), [1, 2, 3])
    with pytest.raises(ValueError):
        job.set_queries(np.zeros((3, 7, 7)), [0.1] * 3, np.ones((3, 6)), [1, 2, 3])
    set_queries(job, qs)
    job.set_shape(64, 4)
    with pytest.raises(S.SsppError, match=E_INVAL + ".*NT = 64"):
        job.sample_score_queries(0, 70, out["arc"], out["feasible"], out["best"])
    job.set_shape(0, 0)
    job.sample_score_queries(0, 70, out["arc"], out["feasible"], out["best"])
    import torch
    torch.cuda.synchronize()
