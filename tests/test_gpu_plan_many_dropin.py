"""SamplingPathPlannerN.plan_many: many plan() queries scored as query launches.

Every result is held to plan() on a fresh planner with the same seed (found, n_feasible, index and
cost equal, the winner's control points bit-equal) and to the CPU oracle on the oracle's own
samples, as tests/test_dropin_sspp.py::test_plan_matches_oracle does it.
"""
import os

import numpy as np
import pytest

from oracle import mjcf_ref
from oracle import oracle as O
from tests.conftest import SCENES

pytestmark = pytest.mark.gpu
ROBOCRANE = os.path.join(SCENES, "robocrane.xml")
QUAT = [0.707, 0, 0, 0.707]


@pytest.fixture(scope="module")
def sp(cuda):
    from sspp import _sspp
    return _sspp


@pytest.fixture(scope="module")
def oscene7():
    return O.Scene(mjcf_ref.load(ROBOCRANE), 0, 7)


def crane_pairs(Q):
    """Q (start, end) pairs across the brick stack at rising heights; the first lies in the floor."""
    starts = np.array([[0.5, 0.15 + 0.003 * k, 0.15 + 0.012 * k] + QUAT for k in range(Q)])
    ends = np.array([[0.5, -0.05 - 0.002 * k, 0.15 + 0.012 * k] + QUAT for k in range(Q)])
    starts[0, 2] = ends[0, 2] = 0.01
    return starts, ends


def oracle_plan(sp, oscene, N, start, end, sigma, limits, B, W, n, seed):
    # initializePath: the oracle's interpolation equals the product's bit for bit
    u = np.array([i / (n - 1) for i in range(n)])
    knots, ctrl0 = O.interpolate(np.array([(1 - t) * start + t * end for t in u]), 3, u)
    ctrl = O.sample_sspp(ctrl0, 3, sigma, limits, seed, 0, B)
    arc, feas = O.sspp_score(oscene, knots, 3, ctrl, W)
    idx, best = O.argmin(arc, feas)
    return dict(n_feasible=int(feas.sum()), index=idx, cost=best, ctrl=ctrl[idx] if idx >= 0 else None, knots=knots)


def assert_matches_oracle(r, o):
    assert r.n_feasible == o["n_feasible"] and r.found == (o["index"] >= 0) and r.index == o["index"]
    if r.found:
        assert abs(r.cost - o["cost"]) <= 1e-12
        np.testing.assert_allclose(r.path.ctrls().T, o["ctrl"], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(r.path.knots(), o["knots"])
    else:
        assert r.cost == np.inf and r.path is None and r.n_feasible == 0


def assert_matches_plan(sp, r, start, end, sigma, limits, B, W, n, seed, N=7):
    fresh = getattr(sp, "SamplingPathPlanner%d" % N)(ROBOCRANE)
    fresh.seed = seed
    ok, paths = fresh.plan(start, end, sigma, limits, sample_count=B, check_points=W, init_points=n)
    assert r.found == ok and r.n_feasible == len(paths) and r.index == fresh.last_best_index
    assert r.cost == fresh.last_best_cost
    if ok:
        assert r.path.ctrls().tobytes() == np.ascontiguousarray(fresh.get_ctrl_pts()).tobytes()


def test_plan_many_equals_plan_and_oracle(sp, oscene7, capfd):
    starts, ends = crane_pairs(5)
    planner = sp.SamplingPathPlanner7(ROBOCRANE)
    res = planner.plan_many(starts, ends, 0.1, np.ones(7), sample_count=512, check_points=64, init_points=10)
    assert len(res) == 5
    for q, r in enumerate(res):
        assert_matches_plan(sp, r, starts[q], ends[q], 0.1, np.ones(7), 512, 64, 10, planner.seed)
        assert_matches_oracle(r, oracle_plan(sp, oscene7, 7, starts[q], ends[q], 0.1, np.ones(7), 512, 64, 10, planner.seed))
    capfd.readouterr()
    found = [r.found for r in res]
    assert not found[0] and any(found)                       # the floor query; some query has a winner
    assert any(0 < r.n_feasible < 512 for r in res)


def test_chunking(sp, oscene7):
    """65 queries: a launch of 64 and a launch of one; every query checked."""
    starts, ends = crane_pairs(65)
    starts[:, 2] = ends[:, 2] = 0.15 + 0.002 * np.arange(65)
    starts[0, 2] = ends[0, 2] = 0.01
    planner = sp.SamplingPathPlanner7(ROBOCRANE)
    res = planner.plan_many(starts, ends, 0.05, np.ones(7), sample_count=64, check_points=16, init_points=6)
    assert len(res) == 65
    for q, r in enumerate(res):
        assert_matches_oracle(r, oracle_plan(sp, oscene7, 7, starts[q], ends[q], 0.05, np.ones(7), 64, 16, 6, planner.seed))
    assert not res[0].found and res[64].found and res[64].n_feasible == 64


def test_per_query_seeds(sp, oscene7):
    starts, ends = crane_pairs(3)
    starts[:] = starts[2]
    ends[:] = ends[2]
    planner = sp.SamplingPathPlanner7(ROBOCRANE)
    kw = dict(sample_count=256, check_points=32, init_points=8)
    seeds = [11, 2 ** 63 + 5, 11]
    res = planner.plan_many(starts, ends, 0.1, np.ones(7), seeds=seeds, **kw)
    for q, r in enumerate(res):
        assert_matches_oracle(r, oracle_plan(sp, oscene7, 7, starts[q], ends[q], 0.1, np.ones(7), 256, 32, 8, seeds[q]))
    assert all(r.found for r in res)
    assert res[0].path.ctrls().tobytes() != res[1].path.ctrls().tobytes()     # other samples
    assert res[0].path.ctrls().tobytes() == res[2].path.ctrls().tobytes()
    same = planner.plan_many(starts[:2], ends[:2], 0.1, np.ones(7), **kw)       # the default: the planner's seed
    assert (same[0].found, same[0].cost, same[0].index, same[0].n_feasible) == \
           (same[1].found, same[1].cost, same[1].index, same[1].n_feasible)
    assert same[0].found and same[0].path.ctrls().tobytes() == same[1].path.ctrls().tobytes()
    assert_matches_oracle(same[0], oracle_plan(sp, oscene7, 7, starts[0], ends[0], 0.1, np.ones(7), 256, 32, 8, planner.seed))


def test_planner_state(sp, oscene7, capfd):
    """plan() after plan_many() and plan_many() after plan() each equal the oracle; plan()'s
    state is the last plan()'s."""
    starts, ends = crane_pairs(4)
    planner = sp.SamplingPathPlanner7(ROBOCRANE)
    args = (0.1, np.ones(7), 256, 32, 8)
    kw = dict(sample_count=256, check_points=32, init_points=8)
    res = planner.plan_many(starts, ends, 0.1, np.ones(7), **kw)
    ok, paths = planner.plan(starts[3], ends[3], 0.1, np.ones(7), **kw)
    o3 = oracle_plan(sp, oscene7, 7, starts[3], ends[3], *args, planner.seed)
    assert ok and len(paths) == o3["n_feasible"] and planner.last_best_index == o3["index"]
    np.testing.assert_allclose(planner.get_ctrl_pts().T, o3["ctrl"], atol=1e-12)
    state = (planner.get_ctrl_pts().tobytes(), planner.last_best_index, planner.last_best_cost,
             list(planner.last_feasible_ids))
    again = planner.plan_many(starts[:3], ends[:3], 0.1, np.ones(7), **kw)
    for q, r in enumerate(again):
        assert_matches_oracle(r, oracle_plan(sp, oscene7, 7, starts[q], ends[q], *args, planner.seed))
        assert (r.found, r.cost, r.index, r.n_feasible) == (res[q].found, res[q].cost, res[q].index, res[q].n_feasible)
    assert state == (planner.get_ctrl_pts().tobytes(), planner.last_best_index, planner.last_best_cost,
                     list(planner.last_feasible_ids))
    assert res[3].index == planner.last_best_index and res[3].path.ctrls().tobytes() == state[0]
    capfd.readouterr()


def test_other_dofs(sp):
    """SamplingPathPlanner3 / 6 / 9 with two queries, in the manner of test_dropin_sspp.py::test_other_dofs."""
    for N in (3, 6, 9):
        planner = getattr(sp, "SamplingPathPlanner%d" % N)(ROBOCRANE)
        q0 = np.array([0.5, 0.15, 0.3, 0.707, 0, 0, 0.707, 0.5, -0.05])[:N]
        q1 = q0.copy()
        q1[1] = -0.05
        starts, ends = np.stack([q0, q0 + 0.01]), np.stack([q1, q1 + 0.01])
        res = planner.plan_many(starts, ends, 0.02, np.ones(N), sample_count=64, check_points=32, init_points=6)
        osc = O.Scene(mjcf_ref.load(ROBOCRANE), 0, N)
        for q, r in enumerate(res):
            assert_matches_oracle(r, oracle_plan(sp, osc, N, starts[q], ends[q], 0.02, np.ones(N), 64, 32, 6, planner.seed))
            assert_matches_plan(sp, r, starts[q], ends[q], 0.02, np.ones(N), 64, 32, 6, planner.seed, N)


def test_argument_errors(sp):
    planner = sp.SamplingPathPlanner7(ROBOCRANE)
    s, e = crane_pairs(3)
    lim = np.ones(7)
    for bad in [lambda: planner.plan_many(s[:, :6], e, 0.1, lim),                 # wrong N
                lambda: planner.plan_many(s, e[:, :6], 0.1, lim),
                lambda: planner.plan_many(s[0], e[0], 0.1, lim),                  # not (Q, N)
                lambda: planner.plan_many(s, e, 0.1, np.ones(6)),
                lambda: planner.plan_many(s[:0], e[:0], 0.1, lim),                # Q == 0
                lambda: planner.plan_many(s, e[:2], 0.1, lim),                    # starts / ends differ in Q
                lambda: planner.plan_many(s, e, 0.1, lim, seeds=[1, 2]),          # seeds differ in Q
                lambda: planner.plan_many(s, e, 0.1, lim, sample_count=0),
                lambda: planner.plan_many(s, e, 0.1, lim, init_points=3),
                lambda: planner.plan_many(s, e, 0.1, lim, check_points=1)]:
        with pytest.raises(ValueError):
            bad()
    # raised before any GPU work: the planner has not even created its device state
    assert planner._timings()["planner_create_us"] == 0.0
