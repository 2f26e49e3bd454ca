"""Re-posing a scene in place (sspp_scene_set_qpos / sspp_scene_set_body_pose) through both planners'
surfaces.  Every expectation is computed at run time by the CPU oracle on a model dict with the same
values edited, and every result is also held, byte for byte, to fresh product objects on an MJCF
file written with those values (tests/scene_update_worlds.py).  Bars, as
tests/test_gpu_plan_many_dropin.py: feasibility, counts and argmin equal; arcs <= 1e-12 against the
oracle; bytes equal against fresh objects.  TaskSpacePlanner costs against the oracle:
<= 1e-12 * max(1, |x|), the bar of tests/test_gpu_parity.py::test_tsp_kernel_forms_identical (the
per-waypoint sums are in the oracle's order; the remaining difference is the arc-length reduction).

robocrane.xml, SamplingPathPlanner7, sigma 0.1, limits 1, seed 0x5EED, 10 control points; the
oracle alone gives (256 x 32): A 106 feasible / argmin 108, N 25 / 222, W2 157 / 114, W1 34 / 206,
F 8 env-env contacts.  The tests assert the oracle's run-time values and that they are not vacuous.
"""
import functools

import numpy as np
import pytest

from oracle import mjcf_ref
from oracle import oracle as O
from tests import scene_update_worlds as Wd

pytestmark = pytest.mark.gpu
SIGMA, LIMITS, SEED, NINIT = 0.1, np.ones(7), 0x5EED, 10
OPT_NPAIRS, OPT_ORDER, OPT_WP_ORDER, OPT_F32, OPT_PREPASS_STATE = 11, 3, 9, 13, 16
# what the oracle alone gives, (feasible, argmin) per (world, B, W): pinned so that the figures quoted
# above and in the tests' non-vacuity checks cannot drift unnoticed
ORACLE_FIGURES = {("A", 256, 32): (106, 108), ("N", 256, 32): (25, 222), ("A", 512, 64): (206, 108), ("N", 512, 64): (44, 222),
                  ("W2", 256, 32): (157, 114), ("W1", 256, 32): (34, 206)}
# stacking.xml, 256 vias around the midpoint (sigma 0.3, bounds T_LO / T_HI), 32 checks: converged per world
STACK_FIGURES = {"A": 48, "S1": 32, "S2": 0}


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def sp(cuda):
    from sspp import _sspp
    return _sspp


@pytest.fixture(scope="module")
def crane_md():
    return mjcf_ref.load(Wd.ROBOCRANE)


@pytest.fixture(scope="module")
def crane(cuda, crane_md, tmp_path_factory):
    """Per world: the rewritten file, the oracle scene on the edited dict, the whole qpos."""
    d = tmp_path_factory.mktemp("crane_worlds")
    out = {}
    for w, edits in Wd.CRANE.items():
        md = Wd.edit_model(crane_md, edits)
        out[w] = dict(xml=Wd.write_xml(Wd.ROBOCRANE, d / (w + ".xml"), edits), oscene=O.Scene(md, 0, 7), md=md,
                      edits=edits, qpos=Wd.qpos_for(crane_md, edits) if all(
                          crane_md["body_jnt_type"][crane_md["body_names"].index(n)] == 0 for n in edits) else None)
    return out


def init_spline(start, end, n=NINIT):
    u = np.array([i / (n - 1) for i in range(n)])
    return O.interpolate(np.array([(1 - t) * start + t * end for t in u]), 3, u)


_memo = {}


def oracle_plan(world, w, start, end, B, W, seed=SEED, count_static=True, first=0):
    """The oracle's plan() in world w (memoised: the tests share the expectations)."""
    key = (w, tuple(start), tuple(end), B, W, seed, count_static, first)
    if key not in _memo:
        knots, ctrl0 = init_spline(np.asarray(start), np.asarray(end))
        ctrl = O.sample_sspp(ctrl0, 3, SIGMA, LIMITS, seed, first, B)
        arc, feas = O.sspp_score(world[w]["oscene"], knots, 3, ctrl, W, count_static=count_static)
        idx, best = O.argmin(arc, feas)
        _memo[key] = dict(arc=arc, feas=feas, n_feasible=int(feas.sum()), index=idx, cost=best, ctrl=ctrl, knots=knots,
                          ctrl0=ctrl0)
    return _memo[key]


def to_world(obj, world, w, md0, by_name=False):
    """Move `obj` (a drop-in planner or an sspp_amd.Scene) to world w from whatever world it is in."""
    if w == "A":
        obj.set_qpos(md0["qpos0"])
        for name, (pos, quat) in ((n, v) for ww in ("W1", "W2") for n, v in Wd.CRANE[ww].items()):
            b = md0["body_names"].index(name)
            obj.set_body_pose(name, md0["body_pos"][b], md0["body_quat"][b])
    elif world[w]["qpos"] is not None and not by_name:
        obj.set_qpos(world[w]["qpos"])
    else:
        for name, (pos, quat) in world[w]["edits"].items():
            b = md0["body_names"].index(name)
            obj.set_body_pose(name, pos, quat if quat is not None else md0["body_quat"][b])


# ------------------------------------------------------------------ 1. plan() on the drop-in planner
def plan_record(planner, B, W, capfd=None):
    ok, paths = planner.plan(Wd.START7, Wd.END7, SIGMA, LIMITS, sample_count=B, check_points=W, init_points=NINIT)
    return dict(ok=ok, n=len(paths), index=planner.last_best_index, cost=planner.last_best_cost,
                ids=list(planner.last_feasible_ids), best=np.ascontiguousarray(planner.get_ctrl_pts()).tobytes() if ok else b"",
                paths=b"".join(np.ascontiguousarray(p.ctrls()).tobytes() for p in paths),
                best_T=np.array(planner.get_ctrl_pts()).T if ok else None)


def assert_plan_is_oracle(r, o):
    assert r["n"] == o["n_feasible"] and r["ok"] == (o["index"] >= 0) and r["index"] == o["index"]
    assert r["ids"] == list(np.flatnonzero(o["feas"]))
    if r["ok"]:
        assert abs(r["cost"] - o["cost"]) <= 1e-12
        np.testing.assert_allclose(r["best_T"], o["ctrl"][o["index"]], rtol=0, atol=1e-12)


def assert_plan_is_fresh(sp, r, xml, B, W):
    fresh = sp.SamplingPathPlanner7(xml)
    f = plan_record(fresh, B, W)
    for k in ("ok", "n", "index", "cost", "ids", "best", "paths"):
        assert r[k] == f[k], k
    return fresh


@pytest.mark.parametrize("B,W", [(256, 32), (512, 64)])
def test_plan_follows_the_world_with_the_query_repeated(sp, crane, crane_md, B, W, capfd):
    planner = sp.SamplingPathPlanner7(Wd.ROBOCRANE)
    recs, npairs = [], []
    for w in ("A", "N", "A"):
        if recs:
            to_world(planner, crane, w, crane_md)
        r = plan_record(planner, B, W)
        o = oracle_plan(crane, w, Wd.START7, Wd.END7, B, W)
        print("world %s %dx%d: oracle %d feasible, argmin %d; product %d, %d" % (w, B, W, o["n_feasible"], o["index"],
                                                                                 r["n"], r["index"]))
        assert (o["n_feasible"], o["index"]) == ORACLE_FIGURES[(w, B, W)]   # (the oracle alone: the docstring's figures)
        assert_plan_is_oracle(r, o)
        fresh = assert_plan_is_fresh(sp, r, crane[w]["xml"], B, W)
        npairs.append(planner._option(OPT_NPAIRS))
        assert npairs[-1] == fresh._option(OPT_NPAIRS)
        assert 0 < r["n"] < B
        recs.append(r)
    capfd.readouterr()
    for k in ("ok", "n", "index", "cost", "ids", "best", "paths"):
        assert recs[0][k] == recs[2][k], k                       # back in A: the same bytes
    assert recs[0]["ids"] != recs[1]["ids"] and recs[1]["n"] < recs[0]["n"]
    # the stale-cull trap: in A the gripper is out of the samples' reach and its pairs are culled
    assert npairs[1] > npairs[0] == npairs[2]
    np.testing.assert_array_equal(planner.get_qpos(), crane_md["qpos0"])


def test_an_update_leaves_plans_own_state(sp, crane, crane_md, capfd):
    planner = sp.SamplingPathPlanner7(Wd.ROBOCRANE)
    plan_record(planner, 256, 32)
    state = (planner.get_ctrl_pts().tobytes(), planner.last_best_index, planner.last_best_cost, list(planner.last_feasible_ids))
    to_world(planner, crane, "N", crane_md)
    assert state == (planner.get_ctrl_pts().tobytes(), planner.last_best_index, planner.last_best_cost,
                     list(planner.last_feasible_ids))
    np.testing.assert_array_equal(planner.get_qpos(), crane["N"]["md"]["qpos0"])
    capfd.readouterr()


# ------------------------------------------------------------------ 2. the C-level surfaces
B2, W2 = 256, 32


def queries3():
    return [(Wd.START7 + np.array([0, 0.004 * k, 0.01 * k, 0, 0, 0, 0]), Wd.END7 + np.array([0, -0.003 * k, 0.01 * k, 0, 0, 0, 0]),
             SEED + 7 * k) for k in range(3)]


class JobSet:
    """A scene with everything test 2 runs on it: the job, its query set, a step executor."""

    def __init__(self, xml, f32):
        import sspp_amd as S
        import torch
        self.S, self.torch = S, torch
        self.scene = S.Scene(S.Model(xml), 0, 7)
        self.knots, self.ctrl0 = init_spline(Wd.START7, Wd.END7)
        self.job = S.SsppJob(self.scene, self.knots, 3, self.ctrl0, SIGMA, LIMITS, W2, seed=SEED, max_batch=B2)
        self.job.set_option(OPT_F32, f32)
        self.steps = 4
        self.arcs = [torch.empty(self.steps * B2, dtype=torch.float64, device="cuda")]
        self.feas = [torch.empty(self.steps * B2, dtype=torch.uint8, device="cuda")]
        self.ex = S.SsppSteps([self.job], [torch.cuda.current_stream()], B2, self.arcs, self.feas, steps_per_launch=self.steps)

    def set_queries(self):
        qs = queries3()
        self.job.set_queries(np.stack([init_spline(s, e)[1] for s, e, _ in qs]), [SIGMA] * 3, np.stack([LIMITS] * 3),
                             [sd for _, _, sd in qs])

    def run(self, ctrl_in):
        """Every launch kind once; numpy outputs."""
        torch, job = self.torch, self.job
        # the read-backs as the scene update (or the creation) left them, before anything else runs
        out = dict(order_first=(job.get_option(OPT_ORDER), job.get_option(OPT_WP_ORDER), job.get_option(OPT_PREPASS_STATE)))
        o = job.alloc(B2, with_ctrl=True)
        job.sample_score(0, B2, o["arc"], o["feasible"], o["best"], ctrl_out=o["ctrl"])
        torch.cuda.synchronize()
        out["sample"] = {k: _np(v) for k, v in o.items()}
        out["f32_ran"] = job.get_option(self.S._lib.OPT_LAST_F32)
        o = job.alloc(B2)
        job.score_ctrl(torch.from_numpy(ctrl_in).cuda(), 0, o["arc"], o["feasible"], o["best"])
        torch.cuda.synchronize()
        out["score"] = {k: _np(v) for k, v in o.items()}
        o = job.alloc_queries(3, B2, with_ctrl=True)
        job.sample_score_queries(0, B2, o["arc"], o["feasible"], o["best"], ctrl_out=o["ctrl"])
        torch.cuda.synchronize()
        out["queries"] = {k: _np(v) for k, v in o.items()}
        out["npairs_q"] = job.get_option(OPT_NPAIRS)
        best = torch.zeros((self.steps, 4), dtype=torch.int64, device="cuda")
        self.ex.enqueue(self.steps, 5 * B2, B2, best)
        torch.cuda.synchronize()
        out["steps"] = dict(arc=_np(self.arcs[0]).copy(), feasible=_np(self.feas[0]).copy(), best=_np(best))
        out["split"] = job.get_option(self.S._lib.OPT_LAST_SPLIT)
        job.update(self.ctrl0, SIGMA, LIMITS, SEED)            # the read-backs below: the job's own table again
        out["npairs"] = job.get_option(OPT_NPAIRS)
        out["order"] = (job.get_option(OPT_ORDER), job.get_option(OPT_WP_ORDER), job.get_option(OPT_PREPASS_STATE))
        return out


def assert_same_bytes(a, b, what):
    for kind in ("sample", "score", "queries", "steps"):
        for k in a[kind]:
            # (control-point rows of infeasible candidates are written too here: whole arrays)
            assert a[kind][k].tobytes() == b[kind][k].tobytes(), (what, kind, k)
    for k in ("npairs", "npairs_q", "f32_ran", "split", "order_first", "order"):
        assert a[k] == b[k], (what, k)


def assert_jobs_are_oracle(S, world, w, out):
    o = oracle_plan(world, w, Wd.START7, Wd.END7, B2, W2)
    for kind in ("sample", "score"):
        g = out[kind]
        np.testing.assert_array_equal(g["feasible"], o["feas"])
        fin = np.isfinite(o["arc"])
        np.testing.assert_array_equal(np.isfinite(g["arc"]), fin)
        assert not fin.any() or np.abs(g["arc"][fin] - o["arc"][fin]).max() <= 1e-12
        cost, idx, cnt = S.decode_best(g["best"])
        assert (idx, cnt) == (o["index"], o["n_feasible"])
    assert np.abs(out["sample"]["ctrl"] - o["ctrl"]).max() <= 1e-12
    for q, (s, e, sd) in enumerate(queries3()):
        oq = oracle_plan(world, w, s, e, B2, W2, seed=sd)
        np.testing.assert_array_equal(out["queries"]["feasible"][q], oq["feas"])
        fin = np.isfinite(oq["arc"])
        assert not fin.any() or np.abs(out["queries"]["arc"][q][fin] - oq["arc"][fin]).max() <= 1e-12
        cost, idx, cnt = S.decode_best(out["queries"]["best"][q])
        assert (idx, cnt) == (oq["index"], oq["n_feasible"])
    for i in range(4):
        f0 = (5 + i) * B2
        os_ = oracle_plan(world, w, Wd.START7, Wd.END7, B2, W2, first=f0)
        sl = slice(i * B2, (i + 1) * B2)
        np.testing.assert_array_equal(out["steps"]["feasible"][sl], os_["feas"])
        fin = np.isfinite(os_["arc"])
        assert not fin.any() or np.abs(out["steps"]["arc"][sl][fin] - os_["arc"][fin]).max() <= 1e-12
        cost, idx, cnt = S.decode_best(out["steps"]["best"][i])
        assert idx == (f0 + os_["index"] if os_["index"] >= 0 else -1) and cnt == os_["n_feasible"]
    return o


@pytest.mark.parametrize("f32", [1, 0])
def test_jobs_queries_and_steps_follow_the_world(crane, crane_md, f32):
    import sspp_amd as S
    js = JobSet(Wd.ROBOCRANE, f32)
    ctrl_in = oracle_plan(crane, "A", Wd.START7, Wd.END7, B2, W2)["ctrl"]
    outs, counts = {}, []
    for step, w in enumerate(("A", "N", "A")):
        js.set_queries()                                         # the set is made before the update ...
        if step:
            to_world(js.scene, crane, w, crane_md)              # ... and launched after it
            assert js.scene.epoch > 0
        out = js.run(ctrl_in)
        o = assert_jobs_are_oracle(S, crane, w, out)
        fresh = JobSet(crane[w]["xml"], f32)
        fresh.set_queries()
        assert_same_bytes(out, fresh.run(ctrl_in), "world %s against fresh objects" % w)
        # the census ran again inside the update: hit order, no asynchronous pre-pass, as at creation
        assert out["f32_ran"] <= f32 and out["order_first"] == (2, 2, 0) == out["order"]
        assert 0 < o["n_feasible"] < B2
        counts.append(o["n_feasible"])
        outs[step] = out
    assert_same_bytes(outs[0], outs[2], "A again")
    assert counts[0] != counts[1] and outs[1]["npairs"] > outs[0]["npairs"]
    assert outs[1]["npairs_q"] > outs[0]["npairs_q"]            # the set's table followed too


# ------------------------------------------------------------------ 3. plan_many
def test_plan_many_before_and_after(sp, crane, crane_md, capfd):
    qs = queries3()
    starts, ends = np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs])
    seeds = [q[2] for q in qs]
    kw = dict(sample_count=256, check_points=32, init_points=NINIT, seeds=seeds)
    planner = sp.SamplingPathPlanner7(Wd.ROBOCRANE)
    got = {}
    for w in ("A", "N"):
        if w != "A":
            to_world(planner, crane, w, crane_md)
        res = planner.plan_many(starts, ends, SIGMA, LIMITS, **kw)
        fresh = sp.SamplingPathPlanner7(crane[w]["xml"]).plan_many(starts, ends, SIGMA, LIMITS, **kw)
        for q, (r, f) in enumerate(zip(res, fresh)):
            o = oracle_plan(crane, w, starts[q], ends[q], 256, 32, seed=seeds[q])
            assert r.n_feasible == o["n_feasible"] and r.found == (o["index"] >= 0) and r.index == o["index"]
            assert (r.found, r.cost, r.index, r.n_feasible) == (f.found, f.cost, f.index, f.n_feasible)
            if r.found:
                assert abs(r.cost - o["cost"]) <= 1e-12
                np.testing.assert_allclose(r.path.ctrls().T, o["ctrl"][o["index"]], rtol=0, atol=1e-12)
                assert r.path.ctrls().tobytes() == f.path.ctrls().tobytes()
        got[w] = [r.n_feasible for r in res]
    capfd.readouterr()
    assert got["A"] != got["N"] and any(0 < n < 256 for n in got["N"])


# ------------------------------------------------------------------ 4. world F: env-env contacts
def oracle_static(oscene):
    """Env-env contacts and cost: the whole scene's with the mover far above everything."""
    far = np.array([0.5, 0.168, 5.0, 0.707, 0, 0, 0.707])
    n_all, c_all, _ = oscene.contacts(far, count_static=True)
    n_mov, _, _ = oscene.contacts(far, count_static=False)
    assert n_mov == 0
    return n_all, c_all


def test_world_f_static_contacts(sp, crane, crane_md, capfd):
    import sspp_amd as S
    import torch
    model = S.Model(Wd.ROBOCRANE)
    scene, loose = S.Scene(model, 0, 7), S.Scene(model, 0, 7, count_static=False)
    assert (scene.info()["static_contacts"], scene.info()["static_cost"]) == oracle_static(crane["A"]["oscene"]) == (0, 0.0)
    for s in (scene, loose):
        to_world(s, crane, "F", crane_md)
    n_o, c_o = oracle_static(crane["F"]["oscene"])
    print("world F: oracle env-env contacts %d, cost %.17g" % (n_o, c_o))
    assert n_o > 0 and c_o < 0.0
    for s in (scene, loose, S.Scene(S.Model(crane["F"]["xml"]), 0, 7)):
        assert (s.info()["static_contacts"], s.info()["static_cost"]) == (n_o, c_o)
    assert n_o == 8 and abs(c_o - -1.3453002310774045) <= 1e-12   # the figures the oracle gave when this was written
    knots, ctrl0 = init_spline(Wd.START7, Wd.END7)
    feas = {}
    for name, s, cs in (("strict", scene, True), ("loose", loose, False)):
        job = S.SsppJob(s, knots, 3, ctrl0, SIGMA, LIMITS, 32, seed=SEED, max_batch=256)
        o = job.alloc(256)
        job.sample_score(0, 256, o["arc"], o["feasible"], o["best"])
        torch.cuda.synchronize()
        want = oracle_plan(crane, "F", Wd.START7, Wd.END7, 256, 32, count_static=cs)
        np.testing.assert_array_equal(_np(o["feasible"]), want["feas"])
        feas[name] = int(want["feas"].sum())
    a = oracle_plan(crane, "A", Wd.START7, Wd.END7, 256, 32)
    assert feas["strict"] == 0 and feas["loose"] == a["n_feasible"] > 0
    # the drop-in planner counts env-env contacts: nothing is feasible in F, and A comes back
    planner = sp.SamplingPathPlanner7(Wd.ROBOCRANE)
    to_world(planner, crane, "F", crane_md)
    assert plan_record(planner, 256, 32)["n"] == 0
    to_world(planner, crane, "A", crane_md)
    assert plan_record(planner, 256, 32)["n"] == a["n_feasible"]
    capfd.readouterr()


# ------------------------------------------------------------------ 5. jointless bodies by name, errors
def test_set_body_pose_by_name_second_scene_errors(sp, crane, crane_md, capfd):
    import sspp_amd as S
    model = S.Model(Wd.ROBOCRANE)
    scene, other = S.Scene(model, 0, 7), S.Scene(model, 0, 7)
    planner = sp.SamplingPathPlanner7(Wd.ROBOCRANE)
    base = oracle_plan(crane, "A", Wd.START7, Wd.END7, 256, 32)
    knots, ctrl0 = init_spline(Wd.START7, Wd.END7)

    def feasible_on(s):
        import torch
        job = S.SsppJob(s, knots, 3, ctrl0, SIGMA, LIMITS, 32, seed=SEED, max_batch=256)
        o = job.alloc(256)
        job.sample_score(0, 256, o["arc"], o["feasible"], o["best"])
        torch.cuda.synchronize()
        return _np(o["feasible"]), _np(o["arc"])

    epoch = 0
    for w in ("W2", "W1"):
        to_world(scene, crane, "A", crane_md)
        to_world(planner, crane, "A", crane_md)
        epoch += 3                                               # set_qpos and two set_body_pose
        to_world(scene, crane, w, crane_md, by_name=True)
        to_world(planner, crane, w, crane_md, by_name=True)
        epoch += 1
        assert scene.epoch == epoch and other.epoch == 0
        o = oracle_plan(crane, w, Wd.START7, Wd.END7, 256, 32)
        print("world %s: oracle %d feasible, argmin %d" % (w, o["n_feasible"], o["index"]))
        assert (o["n_feasible"], o["index"]) == ORACLE_FIGURES[(w, 256, 32)]
        f, arc = feasible_on(scene)
        np.testing.assert_array_equal(f, o["feas"])
        fin = np.isfinite(o["arc"])
        assert np.abs(arc[fin] - o["arc"][fin]).max() <= 1e-12
        ff, farc = feasible_on(S.Scene(S.Model(crane[w]["xml"]), 0, 7))
        assert f.tobytes() == ff.tobytes() and arc.tobytes() == farc.tobytes()
        r = plan_record(planner, 256, 32)
        assert_plan_is_oracle(r, o)
        assert_plan_is_fresh(sp, r, crane[w]["xml"], 256, 32)
        assert 0 < o["n_feasible"] < 256 and o["n_feasible"] != base["n_feasible"]
        # a second scene of the same Model is where it was
        np.testing.assert_array_equal(feasible_on(other)[0], base["feas"])
        np.testing.assert_array_equal(other.qpos(), crane_md["qpos0"])
    # get_qpos round-trips, normalised as the loader normalises
    q = np.array(crane_md["qpos0"])
    q[21:28] = [0.3, -0.2, 0.9, 2.0, 0.0, 0.0, 2.0]
    scene.set_qpos(q)
    want = q.copy()
    want[24:28] = q[24:28] / np.sqrt((q[24:28] ** 2).sum())
    np.testing.assert_array_equal(scene.qpos(), want)
    planner.set_qpos(q)
    np.testing.assert_array_equal(planner.get_qpos(), want)
    # every invalid call raises and changes nothing
    epoch, info = scene.epoch, scene.info()
    f0 = feasible_on(scene)[0]
    bad_q = [q[:-1], np.append(q, 0.0), np.where(np.arange(q.size) == 3, np.nan, q)]
    zq = q.copy()
    zq[3:7] = 0.0
    bad_q.append(zq)
    for b in bad_q:
        with pytest.raises(S.SsppError, match="-1"):
            scene.set_qpos(b)
        with pytest.raises((ValueError, RuntimeError)):
            planner.set_qpos(b)
    for body, pos, quat in ((0, (0, 0, 0), Wd.IDENT), (-3, (0, 0, 0), Wd.IDENT), (10 ** 6, (0, 0, 0), Wd.IDENT),
                            ("blockwall1", (0, 0, 0), (0, 0, 0, 0)), ("blockwall1", (np.inf, 0, 0), Wd.IDENT)):
        with pytest.raises(S.SsppError, match="-1"):
            scene.set_body_pose(body, pos, quat)
    with pytest.raises(S.SsppError):
        scene.set_body_pose("no such body", (0, 0, 0), Wd.IDENT)
    with pytest.raises((ValueError, RuntimeError)):
        planner.set_body_pose("no such body", (0, 0, 0), Wd.IDENT)
    with pytest.raises((ValueError, RuntimeError)):
        planner.set_body_pose("blockwall1", (0, 0, 0), (0, 0, 0, 0))
    assert scene.epoch == epoch and scene.info() == info
    np.testing.assert_array_equal(scene.qpos(), want)
    np.testing.assert_array_equal(planner.get_qpos(), want)
    np.testing.assert_array_equal(feasible_on(scene)[0], f0)
    capfd.readouterr()


# ------------------------------------------------------------------ 6. TaskSpacePlanner on stacking.xml
T_START, T_END = np.array([0.205, 0.0, 0.12, 0.0]), np.array([0.0, 0.0, 0.32, 0.0])
T_LO, T_HI = (-0.5, -0.5, 0.0, -1.6), (0.5, 0.5, 0.6, 1.6)
T_B, T_CP = 256, 32


@pytest.fixture(scope="module")
def stack(cuda, tmp_path_factory):
    d = tmp_path_factory.mktemp("stack_worlds")
    md0 = mjcf_ref.load(Wd.STACKING)
    body = md0["body_names"].index("block1")
    out = dict(md0=md0, body=body)
    for w, edits in Wd.STACK.items():
        md = Wd.edit_model(md0, edits)
        out[w] = dict(xml=Wd.write_xml(Wd.STACKING, d / (w + ".xml"), edits), oscene=O.Scene(md, 1, body), md=md,
                      qpos=Wd.qpos_for(md0, edits))
    return out


def tsp_vias():
    mean = (T_START + 0.5 * (T_END - T_START)).reshape(1, 4)
    return mean, np.full((1, 4), 0.3), O.sample_tsp(mean, np.full((1, 4), 0.3), T_LO, T_HI, 0.0, SEED, 0, T_B)


def close_tsp(a, b):
    fin = np.isfinite(b)
    return np.array_equal(np.isfinite(a), fin) and (np.abs(a[fin] - b[fin]) <= 1e-12 * np.maximum(1.0, np.abs(b[fin]))).all()


def tsp_run(S, scene):
    import torch
    mean, sigma, vias = tsp_vias()
    job = S.TspJob(scene, T_START, T_END, 1, T_CP, mean=mean, sigma=sigma, lo=T_LO, hi=T_HI, seed=SEED, max_batch=T_B)
    out = {}
    o = job.alloc(T_B)
    job.score_vias(torch.from_numpy(vias).cuda(), 0, o["L"], o["Cnf"], o["Cwf"], o["status"], o["cost"], o["best"])
    torch.cuda.synchronize()
    out["vias"] = {k: _np(v) for k, v in o.items()}
    o = job.alloc(T_B, with_vias=True)
    job.sample_score(0, T_B, o["L"], o["Cnf"], o["Cwf"], o["status"], o["cost"], o["best"], vias_out=o["vias"])
    torch.cuda.synchronize()
    out["sample"] = {k: _np(v) for k, v in o.items()}
    return job, out


def test_tsp_jobs_follow_the_world(stack):
    import sspp_amd as S
    model = S.Model(Wd.STACKING)
    scene = S.Scene(model, 1, "block1")
    _, _, vias = tsp_vias()
    conv, costs, stat = {}, {}, {}
    for w in ("A", "S1", "S2", "A"):
        scene.set_qpos(stack[w]["qpos"])
        job, out = tsp_run(S, scene)
        L, Cnf, Cwf, st, cost = O.tsp_score(stack[w]["oscene"], T_START, T_END, vias, T_CP)
        for kind in ("vias", "sample"):
            g = out[kind]
            if kind == "sample":
                assert np.abs(g["vias"] - vias).max() <= 1e-12
            np.testing.assert_array_equal(g["status"], st)
            assert close_tsp(g["L"], L) and close_tsp(g["Cnf"], Cnf) and close_tsp(g["Cwf"], Cwf) and close_tsp(g["cost"], cost)
            assert S.decode_best(g["best"])[1] == O.tsp_best(cost, st)[0]
        _, fresh = tsp_run(S, S.Scene(S.Model(stack[w]["xml"]), 1, "block1"))
        for kind in out:
            for k in out[kind]:
                assert out[kind][k].tobytes() == fresh[kind][k].tobytes(), (w, kind, k)
        # the env-env cost per waypoint: the oracle's whole-scene cost with block1 far from everything
        c_o = stack[w]["oscene"].contacts(np.array([0.45, 0.45, 0.58, 0.0]), count_static=True)[1]
        print("world %s: %d converged, best %d, static cost %.17g" % (w, int(st.sum()), O.tsp_best(cost, st)[0], c_o))
        if w in conv:
            assert conv[w] == int(st.sum()) and np.array_equal(costs[w], cost)
        conv[w], costs[w], stat[w] = int(st.sum()), cost, scene.info()["static_cost"]
        assert abs(stat[w] - c_o) <= 1e-12 * max(1.0, abs(c_o))
        assert stat[w] == S.Scene(S.Model(stack[w]["xml"]), 1, "block1").info()["static_cost"]
    assert 0 < conv["A"] < T_B and 0 < conv["S1"] < T_B and conv["S1"] != conv["A"]
    assert (costs["S1"] != costs["A"]).sum() > 0
    assert conv == STACK_FIGURES and stat["S2"] < stat["A"]
    assert abs(stat["S2"] - -26.648900732844773) <= 1e-12 * 26.7    # (held to the oracle's run-time value above)


def ces_kw():
    return dict(sample_count=T_B - 2, check_points=T_CP, limits_min=T_LO, limits_max=T_HI, seed=SEED)


def ces_read(pl):
    import torch
    torch.cuda.synchronize()
    r = pl.read()
    return {k: (v.tobytes() if hasattr(v, "tobytes") else v) for k, v in r.items()}


def test_ces_planners_follow_the_world(stack):
    import sspp_amd as S
    scene = S.Scene(S.Model(Wd.STACKING), 1, "block1")
    pl = S.CesPlanner(scene, **ces_kw())
    pl.plan(T_START, T_END, iterate=False, iterations=2)       # a warm distribution in world A
    warm = pl.read()
    scene.set_qpos(stack["S1"]["qpos"])
    kept = pl.read()
    for k in ("mean", "sigma", "last_best"):
        np.testing.assert_array_equal(kept[k], warm[k])         # the update keeps the distribution ...
    assert kept["iteration"] == warm["iteration"] and kept["has_best"] == warm["has_best"]
    fscene = S.Scene(S.Model(stack["S1"]["xml"]), 1, "block1")
    # warm: continues from the kept distribution in the new world, as a fresh planner given that state
    pl.plan(T_START, T_END, iterate=True, iterations=2)
    fr = S.CesPlanner(fscene, **ces_kw())
    fr.plan(T_START, T_END, iterate=False, iterations=2)       # (the same iteration count; its state replaced)
    fr.set_state(warm["mean"], warm["sigma"], warm["last_best"], has_best=int(warm["has_best"]))
    fr.plan(T_START, T_END, iterate=True, iterations=2)
    a, b = ces_read(pl), ces_read(fr)
    for k in a:
        assert a[k] == b[k], ("warm", k)
    # cold after an update
    cold, fcold = S.CesPlanner(scene, **ces_kw()), S.CesPlanner(fscene, **ces_kw())
    for p in (cold, fcold):
        p.plan(T_START, T_END, iterate=False, iterations=2)
    a, b = ces_read(cold), ces_read(fcold)
    for k in a:
        assert a[k] == b[k], ("cold", k)
    # against the oracle: the last iteration's candidates in the new world
    rec = O.ces_plan(stack["S1"]["oscene"], T_START, T_END, 2, T_B - 2, T_CP, seed=SEED, lo=T_LO, hi=T_HI)[-1]
    r = cold.read()
    np.testing.assert_array_equal(r["status"], rec["status"])
    assert r["n_success"] == rec["n_success"] and r["best_slot"] == rec["best_slot"]
    assert close_tsp(r["cost"], rec["cost"])
    # a two-goal group after another update equals the two planners run one by one
    scene.set_qpos(stack["A"]["qpos"])
    scene.set_qpos(stack["S1"]["qpos"])
    goals = [(T_START, T_END), (T_START + np.array([0, 0.02, 0, 0]), T_END + np.array([0.03, 0, 0.05, 0]))]
    grp = [S.CesPlanner(scene, **dict(ces_kw(), seed=SEED + g)) for g in range(2)]
    one = [S.CesPlanner(fscene, **dict(ces_kw(), seed=SEED + g)) for g in range(2)]
    S.CesPlanner.plan_group(grp, [g[0] for g in goals], [g[1] for g in goals], iterate=False, iterations=2)
    for p, (s, e) in zip(one, goals):
        p.plan(s, e, iterate=False, iterations=2)
    for g in range(2):
        a, b = ces_read(grp[g]), ces_read(one[g])
        for k in a:
            assert a[k] == b[k], ("group", g, k)


def test_tsp_dropin_set_body_pose(stack, capfd):
    from sspp import _tsp
    kw = dict(sample_count=T_B - 2, check_points=T_CP, limits_min=np.array(T_LO), limits_max=np.array(T_HI), seed=SEED)
    pl = _tsp.TaskSpacePlanner(Wd.STACKING, "block1", **kw)
    pl.plan(T_START, T_END, False)
    (pos, quat), = Wd.STACK["S1"].values()
    pl.set_body_pose("block3", pos, quat)
    np.testing.assert_array_equal(pl.get_qpos(), stack["S1"]["md"]["qpos0"])
    got = pl.plan(T_START, T_END, False)
    fr = _tsp.TaskSpacePlanner(stack["S1"]["xml"], "block1", **kw)
    fr.plan(T_START, T_END, False)                               # (the same number of plan() calls: the same Philox ids)
    want = fr.plan(T_START, T_END, False)
    assert len(got) == len(want) > 0
    for a, b in zip(got, want):
        assert (a.L, a.C_nf, a.C_wf) == (b.L, b.C_nf, b.C_wf)
        assert np.array_equal(np.array(a.via), np.array(b.via))
    assert pl.get_ctrl_pts().tobytes() == fr.get_ctrl_pts().tobytes()
    assert (pl.last_n_success, pl.last_best_slot, pl.last_best_cost) == (fr.last_n_success, fr.last_best_slot, fr.last_best_cost)
    with pytest.raises((ValueError, RuntimeError)):
        pl.set_body_pose("block3", pos, (0, 0, 0, 0))
    with pytest.raises((ValueError, RuntimeError)):
        pl.set_qpos(np.zeros(3))
    np.testing.assert_array_equal(pl.get_qpos(), stack["S1"]["md"]["qpos0"])
    capfd.readouterr()


# ------------------------------------------------------------------ 7. a re-planning loop: orders, memory
def live_resources():
    import ctypes as C
    import gc
    import sspp_amd as S
    gc.collect()
    f = S._lib.lib().__getattr__("sspp_debug_live_resources")
    f.restype, f.argtypes = C.c_int, [C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 3)()
    assert f(out) == 0
    return tuple(out)


def wait_landed(planner):
    """Until the asynchronous pre-pass has its result (about a millisecond of census and host ordering)."""
    import time
    t0 = time.perf_counter()
    while planner._option(OPT_PREPASS_STATE) != 2:
        assert time.perf_counter() - t0 < 5.0, "the pre-pass did not land"
        time.sleep(0.0005)


def orders(planner):
    return planner._option(OPT_ORDER), planner._option(OPT_WP_ORDER), planner._option(OPT_PREPASS_STATE)


def test_replanning_loop_orders_and_flat_device_memory(sp, crane, crane_md, capfd):
    """update, plan, plan, the pre-pass lands, plan — over and over: after an update the planner's
    job is in gap / bisection order with no pre-pass running; its second launch in the new world
    restarts the pre-pass; the launch after it lands scans in hit order; every plan equals the
    oracle; and the device buffers, pinned buffers and events alive stay where they were (the
    buffers a pre-pass replaced are released by the next update)."""
    planner = sp.SamplingPathPlanner7(Wd.ROBOCRANE)
    plan_record(planner, 256, 32)
    wait_landed(planner)
    plan_record(planner, 256, 32)
    assert orders(planner) == (2, 2, 3)                      # the creation's pre-pass, applied
    counts = []
    for i in range(5):
        w = "N" if i % 2 == 0 else "A"
        planner.set_qpos(crane[w]["qpos"] if w == "N" else crane_md["qpos0"])
        assert orders(planner) == (1, 0, 3)                  # gap / bisection, the old pre-pass dropped
        r1 = plan_record(planner, 256, 32)
        assert orders(planner) == (1, 0, 3)                  # one plan per update: no census
        r2 = plan_record(planner, 256, 32)
        assert planner._option(OPT_PREPASS_STATE) in (1, 2)  # the second launch restarted it
        wait_landed(planner)
        r3 = plan_record(planner, 256, 32)
        assert orders(planner) == (2, 2, 3)                  # swapped in: hit order
        o = oracle_plan(crane, w, Wd.START7, Wd.END7, 256, 32)
        for r in (r1, r2, r3):
            assert_plan_is_oracle(r, o)
            for k in ("ok", "n", "index", "cost", "ids", "best", "paths"):
                assert r[k] == r1[k], k                      # the same bytes in every order
        del r1, r2, r3, r
        counts.append(live_resources())
    capfd.readouterr()
    print("live (device, pinned, events) per iteration:", counts)
    assert all(c == counts[0] for c in counts), counts


# ------------------------------------------------------------------ 8. entries inside the driven window
@pytest.mark.parametrize("N,world", [(3, "D3"), (9, "D9")])
def test_driven_window_defaults_follow(sp, crane_md, tmp_path, N, world, capfd):
    """SamplingPathPlanner3 takes block_green's quaternion, SamplingPathPlanner9 block_orange's z and
    quaternion, from qpos: an update of those entries changes the movers' defaults."""
    edits = Wd.DRIVEN[world]
    md = Wd.edit_model(crane_md, edits)
    xml = Wd.write_xml(Wd.ROBOCRANE, tmp_path / "driven.xml", edits)
    start = np.concatenate([Wd.START7, [0.5, -0.05]])[:N]
    end = np.concatenate([Wd.END7, [0.5, -0.05]])[:N]
    lim, B, W = np.ones(N), 256, 32
    u = np.array([i / (NINIT - 1) for i in range(NINIT)])
    knots, ctrl0 = O.interpolate(np.array([(1 - t) * start + t * end for t in u]), 3, u)
    ctrl = O.sample_sspp(ctrl0, 3, SIGMA, lim, SEED, 0, B)
    cls = getattr(sp, "SamplingPathPlanner%d" % N)

    def record(p):
        ok, paths = p.plan(start, end, SIGMA, lim, sample_count=B, check_points=W, init_points=NINIT)
        return (ok, len(paths), p.last_best_index, p.last_best_cost, list(p.last_feasible_ids),
                b"".join(np.ascontiguousarray(q.ctrls()).tobytes() for q in paths))

    planner = cls(Wd.ROBOCRANE)
    feas = {}
    for w, m, path in (("file", crane_md, Wd.ROBOCRANE), (world, md, xml), ("file", crane_md, Wd.ROBOCRANE)):
        if w == world:
            planner.set_qpos(Wd.qpos_for(crane_md, edits))
        elif feas:
            (name, _), = edits.items()
            b = crane_md["body_names"].index(name)
            planner.set_body_pose(name, crane_md["body_pos"][b], crane_md["body_quat"][b])
        r = record(planner)
        arc, f = O.sspp_score(O.Scene(m, 0, N), knots, 3, ctrl, W, count_static=True)
        idx, best = O.argmin(arc, f)
        print("dof %d world %s: oracle %d feasible, argmin %d" % (N, w, int(f.sum()), idx))
        assert (r[0], r[1], r[2]) == (idx >= 0, int(f.sum()), idx) and r[4] == list(np.flatnonzero(f))
        if idx >= 0:
            assert abs(r[3] - best) <= 1e-12
        assert r == record(cls(path))
        assert w not in feas or feas[w].tobytes() == f.tobytes()
        feas[w] = f
    capfd.readouterr()
    assert feas["file"].tobytes() != feas[world].tobytes() and 0 < feas[world].sum() < B


# ------------------------------------------------------------------ 9. the cached planner of sspp_plan_sspp
def test_cached_planner_of_plan_sspp_follows(crane, crane_md):
    import ctypes as C
    import sspp_amd as S
    from sspp_amd._lib import Best, lib
    L = lib()
    p = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    scene = S.Scene(S.Model(Wd.ROBOCRANE), 0, 7)
    B, W = 256, 32
    counts = []
    for w in ("A", "N", "A"):
        if counts:
            to_world(scene, crane, w, crane_md)
        for rep in range(2):                                 # the second call repeats the query on the cached job
            knots, ctrl = np.zeros(NINIT + 4), np.zeros((B, NINIT, 7))
            feas, arc, best = np.zeros(B, np.uint8), np.zeros(B), Best()
            rc = L.sspp_plan_sspp(scene.handle, 7, p(Wd.START7), p(Wd.END7), C.c_double(SIGMA), p(LIMITS), B, W, NINIT,
                                  C.c_uint64(SEED), p(knots), p(ctrl), p(feas, C.c_uint8), p(arc), C.byref(best))
            assert rc == 0, L.sspp_last_error()
            o = oracle_plan(crane, w, Wd.START7, Wd.END7, B, W)
            np.testing.assert_array_equal(feas, o["feas"])
            fin = o["feas"].astype(bool)
            assert np.abs(arc[fin] - o["arc"][fin]).max() <= 1e-12
            assert best.index == o["index"] and best.count == o["n_feasible"]
        counts.append(o["n_feasible"])
    assert counts[0] == counts[2] != counts[1]


# ------------------------------------------------------------------ 10. _tsp: warm plan after an update
def test_tsp_dropin_warm_plan_after_update(stack, capfd):
    """_tsp plan(start, end, True) after set_body_pose continues from the kept distribution in the
    new world: equal to a CesPlanner on a fresh scene of the new world given the state the same
    first iteration leaves in the file's world."""
    import sspp_amd as S
    from sspp import _tsp
    kw = dict(sample_count=T_B - 2, check_points=T_CP, limits_min=np.array(T_LO), limits_max=np.array(T_HI), seed=SEED)
    pl = _tsp.TaskSpacePlanner(Wd.STACKING, "block1", **kw)
    pl.plan(T_START, T_END, False)
    (pos, quat), = Wd.STACK["S1"].values()
    pl.set_body_pose("block3", pos, quat)
    got = pl.plan(T_START, T_END, True)
    ref = S.CesPlanner(S.Scene(S.Model(Wd.STACKING), 1, "block1"), **ces_kw())
    ref.plan(T_START, T_END, iterate=False, iterations=1)
    warm = ref.read()
    fr = S.CesPlanner(S.Scene(S.Model(stack["S1"]["xml"]), 1, "block1"), **ces_kw())
    fr.plan(T_START, T_END, iterate=False, iterations=1)
    fr.set_state(warm["mean"], warm["sigma"], warm["last_best"], has_best=int(warm["has_best"]))
    fr.plan(T_START, T_END, iterate=True, iterations=1)
    r = fr.read()
    ok = np.flatnonzero(r["status"] == 1)
    assert len(got) == len(ok) == r["n_success"] == pl.last_n_success and 0 < len(ok) < T_B
    for c, i in zip(got, ok):
        assert (c.L, c.C_nf, c.C_wf) == (r["L"][i], r["C_nf"][i], r["C_wf"][i])
        assert np.array_equal(np.array(c.via), r["vias"][i])
    np.testing.assert_array_equal(pl.get_current_mean(), r["mean"][0])
    np.testing.assert_array_equal(pl.get_current_stddev(), r["sigma"][0])
    assert pl.last_best_slot == r["best_slot"]
    capfd.readouterr()
