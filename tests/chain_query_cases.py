"""Query sets for an arm's query launches (Chain.sample_score_queries / Chain.plan_many) — TEST
INFRASTRUCTURE ONLY, shared by tests/test_chain_query_cases.py (what the sets hold, on the host) and
tests/test_gpu_chain_queries.py (the device against them).

A set is a list of queries on one arm and one spline shape; a query is one of
  mixed    between two free poses, sigma wide enough that some candidates touch and some do not
  blocked  the touching pose of free_poses as start and end with a small sigma: waypoint 0 is a
           clamped spline's first control point, which the sampler keeps, so every candidate touches
  tie      sigma = 0: every candidate is the initial spline between two free poses, all arcs are
           equal and the lowest id must win
Sigma, limits and seed differ from query to query within a set.
"""
import numpy as np

from tests import chain_host as H
from tests import test_gpu_chain as G

MIXED, BLOCKED, TIE = "mixed", "blocked", "tie"
# arm -> dof, degree and the shape its set is used at: n control points, W check points, B candidates
SETS = {"arm7": dict(D=7, degree=3, n=8, W=40, B=130, first_id=11),
        "arm9": dict(D=9, degree=2, n=6, W=65, B=65, first_id=0),
        "arm3": dict(D=3, degree=3, n=8, W=64, B=64, first_id=2 ** 40 + 5)}
ORDER = (MIXED, BLOCKED, TIE, MIXED)  # (neighbours of every kind on both sides of the blocked and the tie query)
# the two sigmas of an arm's mixed queries (first, second mixed query of a set): at the arm's shape and
# ORDER each gives between a tenth and a third of the candidates feasible
MIXED_SIGMA = {"arm7": (0.05, 0.10), "arm9": (0.10, 0.05), "arm3": (0.30, 0.20)}
POOL_SEEDS = range(77, 93)  # pools of tests/test_gpu_chain.py::free_poses tried in this order
LINE_POINTS = 520  # a free pair is kept when the straight line between its poses is free on this grid
MIN_EACH = 4  # a mixed query has at least this many feasible and this many infeasible candidates

_PATHS = {}


def _paths(exe, tmp, xml, D, count=3):
    """the first `count` (start, end) pairs of free_poses whose straight line in joint space the host
    program finds free (a query's initial spline is that line), and the first pool's touching pose"""
    key = (xml, D)
    if key not in _PATHS:
        free, touching = [], None
        for seed in POOL_SEEDS:
            start, end, touch = G.free_poses(exe, tmp, xml, D, seed=seed)
            touching = touch if touching is None else touching
            t = np.linspace(0.0, 1.0, LINE_POINTS + 1)[:, None]
            hit = H.chain(exe, xml, D, (1 - t) * start + t * end, tmp, tag="line")["hit"]
            if not hit.any():
                free.append((start, end))
            if len(free) == count:
                break
        assert len(free) == count, "too few free paths in the pools"
        _PATHS[key] = (free, touching)
    return _PATHS[key]


def make(S, exe, tmp, xml, arm, order=ORDER, n=None, mixed_sigma=None):
    """the set of `arm` in `order`: dict(kinds, knots, init [Q, n, D], sigma [Q], limits [Q, D],
    seeds [Q], starts / ends [Q, D]).  Query q's initial spline is the linear one between starts[q]
    and ends[q] (Chain.plan_many's initializePath).  mixed_sigma: the mixed queries' two sigmas
    when not the arm's."""
    c = SETS[arm]
    D, degree, n = c["D"], c["degree"], n or c["n"]
    init, sigma, limits, seeds, starts, ends = [], [], [], [], [], []
    knots, mixed = None, 0
    free, touching = _paths(exe, tmp, xml, D)
    for q, kind in enumerate(order):
        if kind == BLOCKED:
            start, end, sg = touching, touching, 0.01
        elif kind == TIE:
            (start, end), sg = free[2], 0.0
        else:
            (start, end), sg = free[mixed % 2], (mixed_sigma or MIXED_SIGMA[arm])[mixed % 2]
            mixed += 1
        knots, c0 = G.linear_ctrl(S, start, end, n, degree)
        init.append(c0)
        sigma.append(sg)
        limits.append(np.full(D, np.pi) * (1.0 - 0.004 * q))
        seeds.append(0xBEEF + 1000003 * q)
        starts.append(start)
        ends.append(end)
    return dict(kinds=list(order), knots=knots, init=np.ascontiguousarray(np.array(init)), sigma=np.array(sigma),
                limits=np.ascontiguousarray(np.array(limits)), seeds=np.array(seeds, dtype=np.uint64),
                starts=np.ascontiguousarray(np.array(starts)), ends=np.ascontiguousarray(np.array(ends)))


def sampled(S, qs, degree, first_id, B):
    """sspp_sample_ctrl_host's candidates [Q, B, n, D] of the set (it samples through a device job)"""
    import ctypes as C

    from sspp_amd import _lib
    Q, n, D = qs["init"].shape
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    out = np.zeros((Q, B, n, D))
    for q in range(Q):
        c0, lim, row = np.ascontiguousarray(qs["init"][q]), np.ascontiguousarray(qs["limits"][q]), np.zeros((B, n, D))
        _lib.check(_lib.lib().sspp_sample_ctrl_host(dp(qs["knots"]), degree, dp(c0), n, D, float(qs["sigma"][q]), dp(lim),
                                                    int(qs["seeds"][q]), int(first_id), B, dp(row)), "sample")
        out[q] = row
    return out
