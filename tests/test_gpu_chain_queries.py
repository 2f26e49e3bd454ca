"""Query launches for arms on the GPU: sspp_chain_sample_score_queries (k_chain_best_q) and
sspp_chain_plan_many_host through Chain.sample_score_queries / Chain.plan_many.

Row q of a query launch is compared byte for byte with Chain.sample_score on query q alone, and with
the independent pieces: sspp_sample_ctrl_host's candidates, the host program's decision at every
waypoint (tests/chain/check_chain.cpp), the scene-less job's arc lengths and numpy's argmin.  The
query sets are those of tests/chain_query_cases.py; what a mixed query holds is asserted from the
host program's decisions before anything is compared with the device.
"""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import chain_host as H
from tests import chain_query_cases as QC
from tests import chain_scenes as W
from tests import test_gpu_chain as G
from tests.test_gpu_chain import S, arms, exe, tmp  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

BIG_ID = 2 ** 40 + 5
E_INVAL = r"\(-1\)"


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _dp(x):
    return x.ctypes.data_as(C.POINTER(C.c_double))


def run_queries(S, ch, qs, degree, Wc, first_id, B, null=()):
    """one query launch into sentinel-filled buffers; `null`: the outputs passed as None"""
    import torch
    Q, n, D = qs["init"].shape
    arc = torch.full((Q, B), -1.0, dtype=torch.float64, device="cuda")
    feas = torch.full((Q, B), 7, dtype=torch.uint8, device="cuda")
    ctrl = None if "ctrl" in null else torch.full((Q, B, n, D), -2.0, dtype=torch.float64, device="cuda")
    best = None if "best" in null else torch.full((Q, 4), -3, dtype=torch.int64, device="cuda")
    bctrl = None if "best_ctrl" in null else torch.full((Q, n, D), -4.0, dtype=torch.float64, device="cuda")
    ch.sample_score_queries(qs["knots"], degree, qs["init"], qs["sigma"], qs["limits"], qs["seeds"], Wc, first_id, B, arc,
                            feas, best=best, ctrl_out=ctrl, best_ctrl=bctrl)
    torch.cuda.synchronize()
    return dict(arc=_np(arc), feasible=_np(feas), ctrl=_np(ctrl), best=_np(best), best_ctrl=_np(bctrl))


def run_single(S, ch, qs, q, degree, Wc, first_id, B):
    """Chain.sample_score on query q alone, into sentinel-filled buffers"""
    import torch
    _, n, D = qs["init"].shape
    arc = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    feas = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    ctrl = torch.full((B, n, D), -2.0, dtype=torch.float64, device="cuda")
    best = torch.full((4,), -3, dtype=torch.int64, device="cuda")
    ch.sample_score(qs["knots"], degree, qs["init"][q], qs["sigma"][q], qs["limits"][q], Wc, first_id, B, arc, feas, best,
                    ctrl_out=ctrl, seed=int(qs["seeds"][q]))
    torch.cuda.synchronize()
    return dict(arc=_np(arc), feasible=_np(feas), ctrl=_np(ctrl), best=_np(best))


def winner_row(single, first_id):
    """the control points of a single-query result's winner, zeros without one"""
    idx = int(single["best"][1])
    return single["ctrl"][idx - first_id] if idx >= 0 else np.zeros_like(single["ctrl"][0])


def assert_rows_equal_singles(S, ch, qs, degree, Wc, first_id, B, null=()):
    got = run_queries(S, ch, qs, degree, Wc, first_id, B, null)
    singles = []
    for q in range(len(qs["kinds"])):
        one = run_single(S, ch, qs, q, degree, Wc, first_id, B)
        singles.append(one)
        where = (q, qs["kinds"][q])
        assert got["arc"][q].tobytes() == one["arc"].tobytes(), where
        assert got["feasible"][q].tobytes() == one["feasible"].tobytes(), where
        assert set(np.unique(one["feasible"])) <= {0, 1}
        if got["ctrl"] is not None:
            assert got["ctrl"][q].tobytes() == one["ctrl"].tobytes(), where
        if got["best"] is not None:
            assert got["best"][q].tobytes() == one["best"].tobytes(), (where, got["best"][q], one["best"])
        if got["best_ctrl"] is not None:
            assert got["best_ctrl"][q].tobytes() == winner_row(one, first_id).tobytes(), where
    return got, singles


def arm_chain(S, arms, arm, count_static=False):
    a = arms(arm)
    return a, S.Chain(a["model"], QC.SETS[arm]["D"], count_static=count_static)


def cycle(Q):
    return tuple(QC.ORDER[q % len(QC.ORDER)] for q in range(Q))


# ------------------------------------------------------------------ 1. rows equal the single-query path
# Q, B, W, n, arm, first_id, outputs passed as null: every Q, B, W and n of the issue, B = 257 past
# k_chain_best_q's 256-thread stride, both first ids, each nullable output null in turn
ROW_CASES = [(1, 1, 40, 4, "arm7", 0, ()), (2, 63, 64, 8, "arm7", 0, ("ctrl",)), (5, 64, 65, 4, "arm7", BIG_ID, ("best",)),
             (64, 65, 40, 4, "arm3", 0, ("best_ctrl",)), (5, 130, 64, 8, "arm7", BIG_ID, ()), (2, 257, 65, 4, "arm7", 0, ()),
             (5, 257, 40, 8, "arm9", BIG_ID, ()), (64, 1, 64, 4, "arm3", BIG_ID, ()), (1, 257, 40, 8, "arm7", 0, ("ctrl",)),
             (2, 64, 40, 4, "arm9", 0, ("best",)), (5, 63, 65, 8, "arm3", 0, ("best_ctrl",)),
             (64, 130, 64, 4, "arm3", BIG_ID, ("ctrl", "best"))]


@pytest.mark.parametrize("Q,B,Wc,n,arm,first_id,null", ROW_CASES)
def test_rows_equal_single_query_path(S, exe, tmp, arms, Q, B, Wc, n, arm, first_id, null):
    a, ch = arm_chain(S, arms, arm)
    order = (QC.MIXED,) if Q == 1 else cycle(Q)
    qs = QC.make(S, exe, tmp, a["xml"], arm, order=order, n=n)
    got, singles = assert_rows_equal_singles(S, ch, qs, QC.SETS[arm]["degree"], Wc, first_id, B, null)
    if Q >= 4 and B >= 63:  # (winners and queries without one both occur in the launch)
        counts = [int(s["best"][2]) for s in singles]
        assert min(counts) == 0 and max(counts) == B


# ------------------------------------------------------------------ 2. rows equal the independent pieces
@pytest.mark.parametrize("arm", sorted(QC.SETS))
def test_rows_equal_independent_pieces(S, exe, tmp, arms, arm):
    c = QC.SETS[arm]
    D, degree, Wc, B, first_id = c["D"], c["degree"], c["W"], c["B"], c["first_id"]
    a, ch = arm_chain(S, arms, arm)
    qs = QC.make(S, exe, tmp, a["xml"], arm)
    want_ctrl = QC.sampled(S, qs, degree, first_id, B)
    want_feas = []
    for q, kind in enumerate(qs["kinds"]):  # what the set holds, from the host program alone
        f, _ = G.host_feasible(S, exe, tmp, a["xml"], D, qs["knots"], degree, want_ctrl[q], Wc, "pieces_%s_%d" % (arm, q))
        print(arm, q, kind, "feasible %d of %d" % (f.sum(), B))
        if kind == QC.MIXED:
            assert f.sum() >= QC.MIN_EACH and (~f).sum() >= QC.MIN_EACH, (arm, q, int(f.sum()))
        elif kind == QC.BLOCKED:
            assert not f.any()
        else:
            assert f.all()
        want_feas.append(f)
    got = run_queries(S, ch, qs, degree, Wc, first_id, B)
    assert got["ctrl"].tobytes() == want_ctrl.tobytes()
    for q in range(len(qs["kinds"])):
        want_arc = G.job_arcs(S, qs["knots"], degree, want_ctrl[q], Wc)
        rec = got["best"][q]
        assert rec[3] == 0
        best = (float(rec[:1].view(np.float64)[0]), int(rec[1]), int(rec[2]))
        G.check_scores(got["arc"][q], got["feasible"][q].astype(bool), best, want_feas[q], want_arc, first_id)
        assert set(np.unique(got["feasible"][q])) <= {0, 1}
        want_row = want_ctrl[q][best[1] - first_id] if best[1] >= 0 else np.zeros_like(want_ctrl[q][0])
        assert got["best_ctrl"][q].tobytes() == want_row.tobytes()


# ------------------------------------------------------------------ 3. neighbours do not leak
def test_neighbours_do_not_leak(S, exe, tmp, arms):
    c = QC.SETS["arm7"]
    degree, Wc, B, first_id = c["degree"], c["W"], c["B"], c["first_id"]
    a, ch = arm_chain(S, arms, "arm7")
    qs = QC.make(S, exe, tmp, a["xml"], "arm7")
    assert qs["kinds"] == [QC.MIXED, QC.BLOCKED, QC.TIE, QC.MIXED]
    got, singles = assert_rows_equal_singles(S, ch, qs, degree, Wc, first_id, B)  # (the outer queries among them)
    blocked, tie = got["best"][1], got["best"][2]
    assert blocked[1] == -1 and np.isposinf(blocked[:1].view(np.float64)[0]) and blocked[2] == 0 and blocked[3] == 0
    assert not got["best_ctrl"][1].any() and got["best_ctrl"][1].tobytes() == np.zeros_like(got["best_ctrl"][1]).tobytes()
    assert not got["feasible"][1].any() and np.all(np.isposinf(got["arc"][1]))
    assert tie[1] == first_id and tie[2] == B and tie[3] == 0
    assert len(set(got["arc"][2].view(np.int64).tolist())) == 1 and got["feasible"][2].all()
    assert got["best_ctrl"][2].tobytes() == qs["init"][2].tobytes()
    for q in (0, 3):
        assert 0 < singles[q]["best"][2] < B


# ------------------------------------------------------------------ 4. static contacts
def test_static_contacts(S, exe, tmp, arms):
    world = G.arm_world(3, 21)  # (test_count_static's world: two overlapping static boxes)
    world["geoms"].append(dict(name="sa", type=W.BOX, size=(0.1, 0.1, 0.1), pos=(3, 3, 0.5)))
    world["bodies"].append(dict(name="gate", pos=(3.15, 3, 0.5), joints=[dict(type="hinge", axis=(0, 0, 1))],
                                geoms=[dict(name="sb", type=W.BOX, size=(0.1, 0.1, 0.1))]))
    model = S.Model(H.write_xml(tmp, "static_q", W.mjcf(world)), joints=True)
    c = QC.SETS["arm3"]
    degree, Wc, B, first_id = c["degree"], c["W"], c["B"], c["first_id"]
    qs = QC.make(S, exe, tmp, arms("arm3")["xml"], "arm3")
    on, off = S.Chain(model, 3, count_static=True), S.Chain(model, 3, count_static=False)
    assert on.info()["static_contacts"] > 0
    g1 = run_queries(S, on, qs, degree, Wc, first_id, B)
    assert not g1["feasible"].any() and np.all(np.isposinf(g1["arc"])) and not g1["best_ctrl"].any()
    assert np.all(g1["best"][:, 1] == -1) and np.all(g1["best"][:, 2] == 0) and np.all(g1["best"][:, 3] == 0)
    assert np.all(np.isposinf(g1["best"][:, 0].copy().view(np.float64)))
    base = S.Chain(arms("arm3")["model"], 3, count_static=True)  # the world without the two boxes
    g0, gb = run_queries(S, off, qs, degree, Wc, first_id, B), run_queries(S, base, qs, degree, Wc, first_id, B)
    assert g0["feasible"].any()
    for k in ("arc", "feasible", "ctrl", "best", "best_ctrl"):
        assert g0[k].tobytes() == gb[k].tobytes(), k


# ------------------------------------------------------------------ 5. single-query state
def test_single_query_state(S, exe, tmp, arms):
    import torch
    c = QC.SETS["arm7"]
    degree, Wc, B, first_id = c["degree"], c["W"], c["B"], c["first_id"]
    a, ch = arm_chain(S, arms, "arm7")
    qs = QC.make(S, exe, tmp, a["xml"], "arm7")
    before = run_single(S, ch, qs, 0, degree, Wc, first_id, B)
    got = run_queries(S, ch, qs, degree, Wc, first_id, B)
    after = run_single(S, ch, qs, 0, degree, Wc, first_id, B)  # (the same values: the job uploads nothing)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    assert got["arc"][0].tobytes() == before["arc"].tobytes()
    # a score_ctrl of another shape replaces the chain's job; the query launch right after it still matches
    other = QC.make(S, exe, tmp, a["xml"], "arm7", n=5)
    arc, feas, best = G.run_score(S, ch, other["knots"], degree, other["init"], Wc + 3)
    assert feas.any()
    again = run_queries(S, ch, qs, degree, Wc, first_id, B)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6. plan_many
PLAN = dict(sigma=0.05, sample_count=65, check_points=40, init_points=8)


def plan_host(S, ch, start, end, limits, seed, sigma, sample_count, check_points, init_points):
    """sspp_chain_plan_host (one query per call): knots, ctrl, feasible, arc, the record"""
    from sspp_amd import _lib
    D, B, n = ch.dof, sample_count, init_points
    knots, ctrl, feas, arc, best = np.zeros(n + 4), np.zeros((B, n, D)), np.zeros(B, np.uint8), np.zeros(B), _lib.Best()
    start, end, limits = (np.ascontiguousarray(x, dtype=np.float64) for x in (start, end, limits))
    _lib.check(_lib.lib().sspp_chain_plan_host(ch.handle, _dp(start), _dp(end), sigma, _dp(limits), B, check_points, n,
                                               int(seed), _dp(knots), _dp(ctrl), feas.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               _dp(arc), C.byref(best)), "chain plan")
    return dict(knots=knots, ctrl=ctrl, feasible=feas, arc=arc, best=(best.cost, best.index, best.count), reserved=best.reserved)


@pytest.mark.parametrize("Q", [3, 65])
def test_plan_many(S, exe, tmp, arms, Q):
    a, ch = arm_chain(S, arms, "arm7", count_static=True)
    qs = QC.make(S, exe, tmp, a["xml"], "arm7", order=cycle(Q))  # (starts and ends: free pairs and the touching pose)
    starts, ends = qs["starts"].copy(), qs["ends"].copy()
    seeds = [0xA11CE + 17 * q for q in range(Q)]
    starts[2], ends[2], seeds[2] = starts[0], ends[0], seeds[0]  # a duplicate of query 0
    limits = np.full(7, np.pi)
    out = ch.plan_many(starts, ends, PLAN["sigma"], limits, PLAN["sample_count"], PLAN["check_points"], PLAN["init_points"],
                       seeds=seeds, return_all=True)
    short = ch.plan_many(starts, ends, PLAN["sigma"], limits, PLAN["sample_count"], PLAN["check_points"], PLAN["init_points"],
                         seeds=seeds)
    assert sorted(short) == ["best", "best_ctrl", "knots", "n_feasible"] and short["best"] == out["best"]
    assert short["best_ctrl"].tobytes() == out["best_ctrl"].tobytes()
    assert out["best_ctrl"].shape == (Q, PLAN["init_points"], 7) and out["arc"].shape == (Q, PLAN["sample_count"])
    winners = 0
    for q in range(Q):
        one = plan_host(S, ch, starts[q], ends[q], limits, seeds[q], **PLAN)
        assert one["reserved"] == 0 and out["knots"].tobytes() == one["knots"].tobytes()
        assert np.array(out["best"][q][:1]).tobytes() == np.array(one["best"][:1]).tobytes() and out["best"][q][1:] == one["best"][1:]
        assert out["n_feasible"][q] == one["best"][2] == int(one["feasible"].sum())
        row = one["ctrl"][one["best"][1]] if one["best"][1] >= 0 else np.zeros_like(one["ctrl"][0])
        assert out["best_ctrl"][q].tobytes() == row.tobytes(), q
        assert out["arc"][q].tobytes() == one["arc"].tobytes() and out["feasible"][q].tobytes() == one["feasible"].tobytes()
        winners += one["best"][1] >= 0
    assert 0 < winners < Q  # (the touching starts have no winner)
    assert out["best"][2] == out["best"][0] and out["best_ctrl"][2].tobytes() == out["best_ctrl"][0].tobytes()
    assert out["arc"][2].tobytes() == out["arc"][0].tobytes() and out["best"][0][1] >= 0


def test_plan_many_first_id(S, exe, tmp, arms):
    """ids [2^40 + 5, ...) at the host level: each query's rows, record and winner row against
    Chain.sample_score on the query alone with the same first id.  The query's initial spline is
    initializePath's own: sspp_chain_plan_host with sigma = 0 returns it as its only candidate."""
    a, ch = arm_chain(S, arms, "arm7", count_static=True)
    qs = QC.make(S, exe, tmp, a["xml"], "arm7")
    limits = np.full(7, np.pi)
    B, Wc, n, Q = PLAN["sample_count"], PLAN["check_points"], PLAN["init_points"], len(qs["kinds"])
    seeds = [0xF00D + 31 * q for q in range(Q)]
    out = ch.plan_many(qs["starts"], qs["ends"], PLAN["sigma"], limits, B, Wc, n, seeds=seeds, first_id=BIG_ID, return_all=True)
    one_set = dict(knots=out["knots"], sigma=np.full(Q, PLAN["sigma"]), limits=np.tile(limits, (Q, 1)), seeds=np.array(seeds),
                   init=np.array([plan_host(S, ch, qs["starts"][q], qs["ends"][q], limits, 0, 0.0, 1, Wc, n)["ctrl"][0]
                                  for q in range(Q)]))
    winners = 0
    for q in range(Q):
        one = run_single(S, ch, one_set, q, 3, Wc, BIG_ID, B)
        cost, idx, cnt = float(one["best"][:1].view(np.float64)[0]), int(one["best"][1]), int(one["best"][2])
        assert out["arc"][q].tobytes() == one["arc"].tobytes() and out["feasible"][q].tobytes() == one["feasible"].tobytes()
        assert np.array(out["best"][q][:1]).tobytes() == np.array([cost]).tobytes() and out["best"][q][1:] == (idx, cnt)
        assert out["n_feasible"][q] == cnt == int(one["feasible"].sum())
        assert idx == -1 or BIG_ID <= idx < BIG_ID + B
        assert out["best_ctrl"][q].tobytes() == winner_row(one, BIG_ID).tobytes(), q
        winners += idx >= 0
    assert 0 < winners < Q


def test_plan_many_default_seeds(S, exe, tmp, arms):
    a, ch = arm_chain(S, arms, "arm7", count_static=True)
    qs = QC.make(S, exe, tmp, a["xml"], "arm7")
    limits = np.full(7, np.pi)
    out = ch.plan_many(qs["starts"], qs["ends"], PLAN["sigma"], limits, PLAN["sample_count"], PLAN["check_points"],
                       PLAN["init_points"])
    for q in range(len(qs["kinds"])):
        one = plan_host(S, ch, qs["starts"][q], qs["ends"][q], limits, S.DEFAULT_SEED, **PLAN)
        assert out["best"][q] == one["best"]


# ------------------------------------------------------------------ 7. ownership
def live(S):
    f = S._lib.lib().__getattr__("sspp_debug_live_resources")
    f.restype, f.argtypes = C.c_int, [C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 3)()
    assert f(out) == 0
    return tuple(out)


def test_ownership(S, exe, tmp, arms):
    a = arms("arm7")
    qs = QC.make(S, exe, tmp, a["xml"], "arm7")
    limits = np.full(7, np.pi)
    gc.collect()
    before = live(S)
    ch = S.Chain(a["model"], 7)
    created = live(S)
    args = (qs["starts"], qs["ends"], PLAN["sigma"], limits, PLAN["sample_count"], PLAN["check_points"], PLAN["init_points"])
    first = ch.plan_many(*args, return_all=True)
    after_first = live(S)
    assert after_first[0] > created[0] and after_first[1] >= created[1] + 4  # (the job, the chunk's buffers, four pinned results)
    for _ in range(3):
        again = ch.plan_many(*args, return_all=True)
        assert live(S) == after_first
        assert again["best"] == first["best"] and again["arc"].tobytes() == first["arc"].tobytes()
    del ch
    gc.collect()
    assert live(S) == before


# ------------------------------------------------------------------ 8. refusals
def test_refusals_device_level(S, exe, tmp, arms):
    import torch
    from sspp_amd import _lib
    c = QC.SETS["arm3"]
    degree, Wc, n, B = c["degree"], c["W"], c["n"], 8
    a, ch = arm_chain(S, arms, "arm3")
    big = QC.make(S, exe, tmp, a["xml"], "arm3", order=cycle(65))
    arc = torch.full((65, B), -1.0, dtype=torch.float64, device="cuda")
    feas = torch.full((65, B), 7, dtype=torch.uint8, device="cuda")
    best = torch.full((65, 4), -3, dtype=torch.int64, device="cuda")
    bctrl = torch.full((65, n, 3), -4.0, dtype=torch.float64, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((arc == -1.0).all() and (feas == 7).all() and (best == -3).all() and (bctrl == -4.0).all())

    def launch(Q):
        ch.sample_score_queries(big["knots"], degree, big["init"][:Q], big["sigma"][:Q], big["limits"][:Q], big["seeds"][:Q],
                                Wc, 0, B, arc, feas, best=best, best_ctrl=bctrl)

    for Q in (0, 65):
        with pytest.raises(S.SsppError, match=E_INVAL + ".*sspp_chain_sample_score_queries"):
            launch(Q)
        assert untouched()
    sig, lim, seeds = big["sigma"][:2].copy(), np.ascontiguousarray(big["limits"][:2]), big["seeds"][:2].copy()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib().sspp_chain_sample_score_queries(ch.handle, _dp(big["knots"]), degree, 2, None, n, Wc, _dp(sig), _dp(lim),
                                                    seeds.ctypes.data_as(C.POINTER(C.c_uint64)), 0, B, vp(arc), vp(feas), None,
                                                    vp(best), vp(bctrl), None)
    assert rc == -1 and "sspp_chain_sample_score_queries" in _lib.last_error() and untouched()
    launch(64)  # (the largest set is served, and B = 0 writes nothing)
    assert not untouched()
    arc.fill_(-1.0), feas.fill_(7), best.fill_(-3), bctrl.fill_(-4.0)
    ch.sample_score_queries(big["knots"], degree, big["init"][:2], sig, lim, seeds, Wc, 0, 0, arc, feas, best=best, best_ctrl=bctrl)
    assert untouched()


def test_refusals_host_level(S, exe, tmp, arms):
    from sspp_amd import _lib
    a, ch = arm_chain(S, arms, "arm7")
    qs = QC.make(S, exe, tmp, a["xml"], "arm7")
    limits = np.full(7, np.pi)
    ok = dict(sample_count=16, check_points=20, init_points=5)
    for Q, bad in ((0, {}), (4, dict(init_points=3)), (4, dict(check_points=1)), (4, dict(sample_count=0))):
        kw = dict(ok, **bad)
        with pytest.raises(S.SsppError, match=E_INVAL + ".*sspp_chain_plan_many_host"):
            ch.plan_many(qs["starts"][:Q], qs["ends"][:Q], 0.1, limits, **kw)
        # the same through the C call, into sentinel-filled outputs: nothing is written
        n, B = max(kw["init_points"], 4), max(kw["sample_count"], 1)
        knots, bc = np.full(n + 4, -5.0), np.full((4, n, 7), -4.0)
        best = np.full((4, 4), -3, dtype=np.int64)
        nf, arc, feas = np.full(4, -6, dtype=np.int64), np.full((4, B), -1.0), np.full((4, B), 7, dtype=np.uint8)
        seeds = np.arange(4, dtype=np.uint64)
        rc = _lib.lib().sspp_chain_plan_many_host(ch.handle, Q, _dp(qs["starts"]), _dp(qs["ends"]), 0.1, _dp(limits),
                                                  kw["sample_count"], kw["check_points"], kw["init_points"],
                                                  seeds.ctypes.data_as(C.POINTER(C.c_uint64)), 0, _dp(knots),
                                                  best.ctypes.data_as(C.POINTER(_lib.Best)), _dp(bc),
                                                  nf.ctypes.data_as(C.POINTER(C.c_int64)), _dp(arc),
                                                  feas.ctypes.data_as(C.POINTER(C.c_uint8)))
        assert rc == -1 and "sspp_chain_plan_many_host" in _lib.last_error()
        assert (knots == -5.0).all() and (bc == -4.0).all() and (best == -3).all() and (nf == -6).all()
        assert (arc == -1.0).all() and (feas == 7).all()
    out = ch.plan_many(qs["starts"], qs["ends"], 0.1, limits, **ok)  # (the chain still serves a good call)
    assert len(out["best"]) == 4
