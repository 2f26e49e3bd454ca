"""Who owns the library's GPU resources: every object gives back exactly what it took.

The owning types (sspp_amd/csrc/sspp_own.h) count the device buffers, pinned buffers and events alive
in the process; sspp_debug_live_resources reads the three counts.  Each case reads them, creates and
uses an object so that every allocation path of its kind runs, checks that the counts rose, drops the
object and asserts that all three counts are what they were — a comparison within the case, since
other tests share the process.  (torch's own allocations are not counted.)
"""
import ctypes as C
import gc
import os

import numpy as np
import pytest

from tests import synth_scenes as Y
from tests.conftest import SCENES

pytestmark = pytest.mark.gpu
ROBOCRANE = os.path.join(SCENES, "robocrane.xml")
STACKING = os.path.join(SCENES, "stacking.xml")
QUAT = [0.707, 0, 0, 0.707]
B = 256


def live():
    import sspp_amd as S
    f = S._lib.lib().__getattr__("sspp_debug_live_resources")
    f.restype, f.argtypes = C.c_int, [C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 3)()
    assert f(out) == 0
    return tuple(out)


def settled():
    """The counts once nothing collectable is left."""
    gc.collect()
    return live()


def rose(now, before, dev=1, pinned=0, events=0):
    return now[0] >= before[0] + dev and now[1] >= before[1] + pinned and now[2] >= before[2] + events


def write_scene(tmp_path, name, xml):
    path = str(tmp_path / (name + ".xml"))
    with open(path, "w") as f:
        f.write(xml)
    return path


def linear(start, end, n=10):
    import sspp_amd as S
    u = np.array([i / (n - 1) for i in range(n)])
    return S.interpolate(np.array([(1 - t) * start + t * end for t in u]), 3, u)


def test_scene_with_and_without_pairs(cuda, tmp_path):
    import sspp_amd as S
    before = settled()
    scene = S.Scene(S.Model(ROBOCRANE), 0, 7)
    assert scene.info()["n_pairs"] > 0
    assert live() == (before[0] + 4, before[1], before[2])  # geoms, pairs, movers, the visit order
    del scene
    assert settled() == before
    # the mover's geom (2 / 2) and the static box (1 / 1) share no collision bit: no pairs
    xml = Y.mjcf([Y.geom(Y.BOX, (0.1, 0.1, 0.1), (0.5, 0, 0.1), name="slab")],
                 [Y.body("mover", (0, 0, 0.3), [Y.geom(Y.BOX, Y.MOVER_BOX, name="m_box", contype=2, conaffinity=2)])])
    scene = S.Scene(S.Model(write_scene(tmp_path, "no_pairs", xml)), 0, 7)
    assert scene.info()["n_pairs"] == 0
    assert live() == (before[0] + 2, before[1], before[2])  # geoms and movers only
    del scene
    assert settled() == before


def test_sspp_job_every_allocation_path(cuda, tmp_path):
    import sspp_amd as S
    import torch
    L = S._lib
    scene = S.Scene(S.Model(write_scene(tmp_path, "boxes", Y.one_type("boxes"))), 0, 7)
    knots, ctrl0 = linear(Y.ONE_START, Y.ONE_END)
    before = settled()
    big = 4096
    job = S.SsppJob(scene, knots, 3, ctrl0, 0.12, Y.ZOO_LIMITS, 64, seed=7, max_batch=big)  # sigma > 0: the census
    assert job.get_option(L.OPT_ORDER) == 2 and job.get_option(L.OPT_WP_ORDER) == 2
    created = live()
    assert rose(created, before, dev=8)
    out = job.alloc(B)
    job.sample_score(0, B, out["arc"], out["feasible"], out["best"])
    _, ctrl1 = linear(Y.ONE_START + np.array([0, 0.01, 0, 0, 0, 0, 0]), Y.ONE_END)
    job.update(ctrl1, 0.1, Y.ZOO_LIMITS, seed=9)  # the pinned staging and its event
    job.sample_score(0, B, out["arc"], out["feasible"], out["best"])
    assert rose(live(), created, dev=0, pinned=1, events=1)
    qs = np.stack([ctrl0, ctrl1, ctrl0])
    job.set_queries(qs, [0.12, 0.1, 0.05], np.tile(Y.ZOO_LIMITS, (3, 1)), [1, 2, 3])
    q = job.alloc_queries(3, B)
    job.sample_score_queries(0, B, q["arc"], q["feasible"], q["best"])
    torch.cuda.synchronize()
    assert job.get_option(L.OPT_LAST_QUERIES) == 3
    assert rose(live(), created, dev=2, pinned=2, events=2)  # the set's values and pair table; its staging
    for order in (0, 1):  # re-uploads the waypoint rows and both tables
        job.set_option(L.OPT_ORDER, order)
        assert job.get_option(L.OPT_ORDER) == order
        job.sample_score(0, B, out["arc"], out["feasible"], out["best"])
    # 2 steps x 4096 in the latency shape: 2048 workgroup records, more than the job's 1024
    st = torch.cuda.current_stream()
    arcs = [torch.empty(4 * big, dtype=torch.float64, device="cuda")]
    feas = [torch.empty(4 * big, dtype=torch.uint8, device="cuda")]
    best = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
    grow = S.SsppSteps([job], [st], big, arcs, feas, steps_per_launch=2)
    grow.enqueue(2, 0, big, best)
    torch.cuda.synchronize()
    assert job.config()["shape"] == "256x64" and job.get_option(L.OPT_LAST_SPLIT) == 0
    split = S.SsppSteps([job], [st], big, arcs, feas, steps_per_launch=4)
    n_before_split = live()
    split.enqueue(4, 0, big, best)
    torch.cuda.synchronize()
    assert job.get_option(L.OPT_LAST_SPLIT) == 1
    assert rose(live(), n_before_split, dev=6)  # the survivor queue
    del grow, split, job
    assert settled() == before
    del scene


class CPlanner:
    """The drop-in planner's C interface (sspp_planner_*), which also reads its plan() job's options."""

    def __init__(self, scene, dof=7):
        import sspp_amd as S
        self.L, self.D = S._lib.lib(), dof
        self.h = C.c_void_p()
        S._lib.check(self.L.sspp_planner_create(scene.handle, dof, C.byref(self.h)), "planner create")

    def plan(self, start, end, sigma=0.1, W=64, n=10):
        import sspp_amd as S
        s, e, lim = (np.ascontiguousarray(a, dtype=np.float64) for a in (start, end, np.ones(self.D)))
        knots, nf, best = np.zeros(n + 4), C.c_int64(), S._lib.Best()
        S._lib.check(self.L.sspp_planner_plan(self.h, S.runtime._dptr(s), S.runtime._dptr(e), sigma, S.runtime._dptr(lim),
                                              B, W, n, 0x5EED, 0, S.runtime._dptr(knots), C.byref(nf), None, None, None,
                                              C.byref(best)), "plan")
        return knots, nf.value

    def option(self, key):
        import sspp_amd as S
        v = C.c_int64()
        S._lib.check(self.L.sspp_planner_get_option(self.h, key, C.byref(v)), "planner option")
        return v.value

    def score(self, knots, ctrl, W=64):
        import sspp_amd as S
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
        arc, feas, best = np.zeros(1), np.zeros(1, np.uint8), S._lib.Best()
        S._lib.check(self.L.sspp_planner_score(self.h, S.runtime._dptr(knots), 3, S.runtime._dptr(ctrl), 1, ctrl.shape[0], W,
                                               1, S.runtime._dptr(arc), feas.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               C.byref(best)), "score")
        return arc[0]

    def plan_many(self, starts, ends, sigma=0.1, W=64, n=10):
        import sspp_amd as S
        s, e, lim = (np.ascontiguousarray(a, dtype=np.float64) for a in (starts, ends, np.ones(self.D)))
        Q = s.shape[0]
        knots, ctrl, nf = np.zeros(n + 4), np.zeros((Q, n, self.D)), np.zeros(Q, np.int64)
        seeds, best = np.full(Q, 0x5EED, np.uint64), (S._lib.Best * Q)()
        S._lib.check(self.L.sspp_planner_plan_many(self.h, Q, S.runtime._dptr(s), S.runtime._dptr(e), sigma,
                                                   S.runtime._dptr(lim), B, W, n, seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   0, S.runtime._dptr(knots), best, S.runtime._dptr(ctrl),
                                                   nf.ctypes.data_as(C.POINTER(C.c_int64)), None, None), "plan_many")
        return nf

    def free(self):
        self.L.sspp_planner_free(self.h)
        self.h = None


def crane_queries(Q):
    starts = np.array([[0.5, 0.15 + 0.003 * k, 0.15 + 0.012 * k] + QUAT for k in range(Q)])
    ends = np.array([[0.5, -0.05 - 0.002 * k, 0.15 + 0.012 * k] + QUAT for k in range(Q)])
    return starts, ends


def test_dropin_planner_with_applied_prepass(cuda):
    import sspp_amd as S
    starts, ends = crane_queries(3)
    before = settled()
    scene = S.Scene(S.Model(ROBOCRANE), 0, 7)
    p = CPlanner(scene)
    knots, _ = p.plan(starts[1], ends[1])
    first = live()
    assert rose(first, before, dev=12, pinned=5, events=1)  # (the pre-pass's event, its pinned hit bits)
    # the pre-pass lands on its own stream and thread; the plan() after that swaps its tables in and
    # retires the replaced ones (state 3).  Each plan() is a launch and a stream wait: no sleeping
    for _ in range(200000):
        if p.option(S._lib.OPT_PREPASS_STATE) == 3:
            break
        p.plan(starts[1], ends[1])
    assert p.option(S._lib.OPT_PREPASS_STATE) == 3
    assert p.option(S._lib.OPT_WP_ORDER) == 2
    assert live()[0] > first[0]  # the retired tables stay alive beside their replacements
    _, ctrl0 = linear(starts[1], ends[1])
    assert p.score(knots, ctrl0) > 0.0  # (+inf when the straight path collides)
    nf = p.plan_many(starts, ends)
    assert nf.shape == (3,) and (nf >= 0).all()
    p.free()
    del scene
    assert settled() == before


def test_dropin_planner_freed_under_its_prepass(cuda):
    import sspp_amd as S
    starts, ends = crane_queries(2)
    before = settled()
    scene = S.Scene(S.Model(ROBOCRANE), 0, 7)
    p = CPlanner(scene)
    p.plan(starts[1], ends[1])
    assert rose(live(), before, dev=12, pinned=5, events=1)
    p.free()  # joins the pre-pass's thread and drops its result
    del scene
    assert settled() == before


@pytest.mark.parametrize("xml,body,form", [(ROBOCRANE, "gripper_collision_with_block/", 2), (STACKING, "block1", -1)],
                         ids=["gripper_pair_split", "stacking_default_form"])
def test_tsp_job(cuda, xml, body, form):
    """48 gripper pairs with the multi-workgroup pair split (its records are allocated at the first
    such launch), and the stacking scene's few pairs at the library's own choice of form."""
    import sspp_amd as S
    import torch
    model = S.Model(xml)
    scene = S.Scene(model, 1, model.body_id(body))
    if form == 2:
        assert scene.info()["n_pairs"] > 8
        start, end = np.array([0.5, 0.15, 0.156, 1.5708]), np.array([0.5, -0.05, 0.156, 1.5708])
        lo, hi = (0.0, -0.7, 0.1, -1.6), (0.7, 0.7, 0.6, 1.6)
    else:
        start = model.body_point("block1") + np.array([0, 0, 0.02, 0])
        end = model.body_point("block2") + np.array([0, 0, 0.22, 0])
        lo, hi = (-0.5, -0.5, 0.0, -1.6), (0.5, 0.5, 0.6, 1.6)
    before = settled()
    job = S.TspJob(scene, start, end, 1, 40, mean=(start + 0.5 * (end - start)).reshape(1, 4), sigma=np.full((1, 4), 0.15),
                   lo=np.array(lo), hi=np.array(hi), max_batch=B)
    created = live()
    assert rose(created, before, dev=8)
    job.set_option(S.OPT_TSP_FORM, form)
    q = job.alloc(B)
    job.sample_score(0, B, q["L"], q["Cnf"], q["Cwf"], q["status"], q["cost"], q["best"])
    torch.cuda.synchronize()
    if form == 2:
        assert job.get_option(S.OPT_TSP_FORM) == 2
        assert live() == (created[0] + 3, created[1], created[2])  # the k_tsp_pp2 records
        job.sample_score(B, B, q["L"], q["Cnf"], q["Cwf"], q["status"], q["cost"], q["best"])
        torch.cuda.synchronize()
        assert live() == (created[0] + 3, created[1], created[2])
    else:
        assert live() == created
    del job
    assert settled() == before
    del scene


def test_ces_planner(cuda):
    import sspp_amd as S
    model = S.Model(STACKING)
    scene = S.Scene(model, 1, model.body_id("block1"))
    before = settled()
    pl = S.CesPlanner(scene, sample_count=B - 2, check_points=64, limits_min=(-0.5, -0.5, 0.0, -1.6),
                      limits_max=(0.5, 0.5, 0.6, 1.6))
    assert rose(live(), before, dev=17 + 8, pinned=1)  # its own 17 buffers, its job's, the staging
    st = model.body_point("block1") + np.array([0, 0, 0.02, 0])
    en = model.body_point("block2") + np.array([0, 0, 0.22, 0])
    pl.plan(st, en, iterate=False, iterations=2)
    r = pl.read()
    assert r["iteration"] == 2 and r["n_candidates"] >= B - 2
    del pl
    assert settled() == before
    del scene


def test_steps_over_two_jobs(cuda, tmp_path):
    import sspp_amd as S
    import torch
    scene = S.Scene(S.Model(write_scene(tmp_path, "boxes", Y.one_type("boxes"))), 0, 7)
    knots, ctrl0 = linear(Y.ONE_START, Y.ONE_END)
    before = settled()
    jobs = [S.SsppJob(scene, knots, 3, ctrl0, 0.12, Y.ZOO_LIMITS, 64, seed=7 + i, max_batch=B) for i in range(2)]
    made = live()
    assert rose(made, before, dev=16)
    streams = [torch.cuda.Stream() for _ in jobs]
    arcs = [torch.empty(2 * B, dtype=torch.float64, device="cuda") for _ in jobs]
    feas = [torch.empty(2 * B, dtype=torch.uint8, device="cuda") for _ in jobs]
    best = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    ex = S.SsppSteps(jobs, streams, B, arcs, feas, steps_per_launch=2)
    assert live() == made  # the executor owns no GPU resource
    ex.enqueue(8, 0, B, best)
    torch.cuda.synchronize()
    assert (best.cpu().numpy()[:, 2] >= 0).all()
    del ex, jobs
    assert settled() == before
    del scene
