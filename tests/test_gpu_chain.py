"""Articulated movers on the GPU (sspp_chain_fk / _contacts / _score_ctrl / _sample_score, the Chain
class and the drop-in planner of an arm) against the stand-alone host program byte for byte
(tests/chain/check_chain.cpp runs the same __host__ __device__ routines), against the scene-less
job's arc lengths bit for bit, and against numpy's argmin.  The host program itself is checked
against tests/chain_ref.py in tests/test_chain_host.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import chain_host as H
from tests import chain_ref as R
from tests import chain_scenes as W
from tests import test_chain_host as TH

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def S(cuda):
    import sspp_amd
    return sspp_amd


@pytest.fixture(scope="module")
def exe(cuda, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chain_gpu") / "check_chain")
    r = H.build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("chain_gpu_worlds")


# (name, world, nq, free base): arms with nq = D, nq > D (the 9-joint arm under every D) and a free base
def arm_world(nj, seed, free_base=False):
    return W.capsule_arm_world(nj, seed, free_base)


ARMS = {"arm3": (3, 21, False), "arm6": (6, 22, False), "arm7": (7, 11, False), "arm9": (9, 23, False),
        "base2": (2, 24, True)}
# (arm, D): nq = D for each D, nq > D on the 9-joint arm, a free base with 0, 2 of its joints driven and
# with only part of the base driven
FK_CASES = [("arm3", 3), ("arm6", 6), ("arm7", 7), ("arm9", 9), ("arm9", 3), ("arm9", 6), ("arm9", 7), ("base2", 9),
            ("base2", 7), ("base2", 6), ("base2", 3)]
N_SIZES = (1, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def arms(S, tmp):
    made = {}

    def get(name):
        if name not in made:
            nj, seed, fb = ARMS[name]
            world = arm_world(nj, seed, fb)
            xml = H.write_xml(tmp, name, W.mjcf(world))
            made[name] = dict(world=world, xml=xml, model=S.Model(xml, joints=True), fb=fb, seed=seed)
        return made[name]

    return get


@pytest.mark.parametrize("name,D", FK_CASES)
def test_fk_and_contacts_equal_host_bytes(S, exe, tmp, arms, name, D):
    import torch
    a = arms(name)
    q = W.arm_poses(D, max(N_SIZES), a["seed"] + 7, 2.0, a["fb"])
    host = H.chain(exe, a["xml"], D, q, tmp, tag="%s_%d" % (name, D))
    assert host["rc"] == 0, host["err"]
    ch = S.Chain(a["model"], D, count_static=False)
    info = ch.info()
    assert {k: info[k] for k in host["info"]} == host["info"] and info["dof"] == D
    assert [(p["geom1"], p["geom2"], int(p["moving1"]), int(p["moving2"]), p["margin"]) for p in ch.pairs()] == host["pairs"]
    assert 0.02 < host["hit"].mean() < 0.95  # (both decisions occur)
    dq = torch.as_tensor(q, device="cuda")
    for N in N_SIZES:
        gpos, gmat = ch.fk(dq[:N])
        got = np.concatenate([_np(gpos), _np(gmat)], 2)
        assert got.tobytes() == host["fk"][:N].tobytes(), (name, D, N, np.abs(got - host["fk"][:N]).max())
        hit = _np(ch.contacts(dq[:N]))
        assert hit.tobytes() == host["hit"][:N].tobytes(), (name, D, N)
    assert _np(ch.contacts(dq[:0])).size == 0


# ------------------------------------------------------------------ score_ctrl
def linear_ctrl(S, start, end, n, degree):
    u = np.linspace(0.0, 1.0, n)
    return S.interpolate(np.array([(1 - t) * start + t * end for t in u]), degree, u)


def host_feasible(S, exe, tmp, xml, D, knots, degree, ctrl, Wc, tag, count_static=0):
    """any waypoint in contact by the host routine at sspp_spline_eval(u = i / W), per candidate"""
    B = len(ctrl)
    q = np.array([[S.spline_eval(knots, degree, ctrl[b], i / Wc) for i in range(Wc + 1)] for b in range(B)])
    host = H.chain(exe, xml, D, q.reshape(-1, D), tmp, count_static=count_static, tag=tag)
    assert host["rc"] == 0, host["err"]
    return ~host["hit"].reshape(B, Wc + 1).astype(bool).any(1), host["hit"].reshape(B, Wc + 1)


def job_arcs(S, knots, degree, ctrl, Wc):
    """the scene-less job's arc lengths (sspp_score_ctrl_host with no scene)"""
    from sspp_amd import _lib
    B, n, D = ctrl.shape
    arc, feas, best = np.zeros(B), np.zeros(B, np.uint8), _lib.Best()
    c = np.ascontiguousarray(ctrl)
    _lib.check(_lib.lib().sspp_score_ctrl_host(None, knots.ctypes.data_as(C.POINTER(C.c_double)), degree,
                                               c.ctypes.data_as(C.POINTER(C.c_double)), B, n, D, Wc,
                                               arc.ctypes.data_as(C.POINTER(C.c_double)),
                                               feas.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(best)), "arcs")
    return arc


def run_score(S, ch, knots, degree, ctrl, Wc, first_id=0):
    import torch
    B = len(ctrl)
    arc = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    feas = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
    best = S.best_tensor()
    ch.score_ctrl(knots, degree, torch.as_tensor(np.ascontiguousarray(ctrl), device="cuda"), Wc, first_id, arc, feas, best)
    torch.cuda.synchronize()
    return _np(arc), _np(feas).astype(bool), S.decode_best(best)


def check_scores(arc, feas, best, want_feas, want_arc, first_id=0):
    np.testing.assert_array_equal(feas, want_feas)
    assert np.array_equal(arc[want_feas].view(np.int64), want_arc[want_feas].view(np.int64))
    assert np.all(np.isposinf(arc[~want_feas]))
    cost, idx, cnt = best
    assert cnt == int(want_feas.sum())
    if cnt:
        k = int(np.flatnonzero(want_feas)[np.argmin(want_arc[want_feas])])  # (argmin: the first of equal arcs)
        assert idx == first_id + k and cost == want_arc[k]
    else:
        assert idx == -1 and np.isposinf(cost)


def free_poses(exe, tmp, xml, D, seed=77):
    """(start, end, a touching pose): two nearby poses the host routine finds free, from a pool"""
    pool = W.arm_poses(D, 400, seed, 1.2)
    hit = H.chain(exe, xml, D, pool, tmp, tag="pool")["hit"].astype(bool)
    free = pool[~hit]
    start = free[0]
    return start, free[np.argsort(np.abs(free - start).max(1))[3]], pool[hit][0]


def random_splines(S, exe, tmp, xml, D, B, n, degree, seed, sigma=0.25):
    """B splines around the linear path between two free poses: noise wide enough that some touch"""
    rng = np.random.default_rng(seed)
    start, end, _ = free_poses(exe, tmp, xml, D)
    knots, c0 = linear_ctrl(S, start, end, n, degree)
    noise = rng.normal(0.0, sigma, (B, n, D)) * rng.uniform(0.0, 2.0, (B, 1, 1))
    for d in range(D):
        if d % 3 == 2:  # (a slide: metres)
            noise[:, :, d] *= 0.15
    return knots, np.ascontiguousarray(c0[None] + noise)


SCORE_CASES = [(1, 1, 4, 3, "arm7"), (63, 63, 10, 3, "arm7"), (64, 64, 4, 3, "arm7"), (65, 65, 10, 3, "arm7"),
               (200, 128, 4, 3, "arm7"), (64, 128, 10, 3, "arm6"), (65, 1, 10, 3, "arm3"), (200, 63, 10, 2, "arm9")]


@pytest.mark.parametrize("B,Wc,n,degree,arm", SCORE_CASES)
def test_score_ctrl(S, exe, tmp, arms, B, Wc, n, degree, arm):
    a = arms(arm)
    D = ARMS[arm][0]
    ch = S.Chain(a["model"], D, count_static=False)
    knots, ctrl = random_splines(S, exe, tmp, a["xml"], D, B, n, degree, 1000 + B + Wc)
    if B == 1:  # (a batch of one cannot mix: both kinds, one after the other)
        pool_k, pool = random_splines(S, exe, tmp, a["xml"], D, 64, n, degree, 5)
        f, _ = host_feasible(S, exe, tmp, a["xml"], D, pool_k, degree, pool, Wc, "pool")
        assert f.any() and not f.all()
        for pick in (int(np.flatnonzero(f)[0]), int(np.flatnonzero(~f)[0])):
            arc, feas, best = run_score(S, ch, pool_k, degree, pool[pick:pick + 1], Wc, first_id=17)
            check_scores(arc, feas, best, f[pick:pick + 1], job_arcs(S, pool_k, degree, pool[pick:pick + 1], Wc), 17)
        return
    want_feas, _ = host_feasible(S, exe, tmp, a["xml"], D, knots, degree, ctrl, Wc, "score")
    assert want_feas.any() and not want_feas.all()
    arc, feas, best = run_score(S, ch, knots, degree, ctrl, Wc, first_id=5)
    check_scores(arc, feas, best, want_feas, job_arcs(S, knots, degree, ctrl, Wc), 5)


@pytest.mark.parametrize("Wc", [64, 65, 128])
def test_score_ctrl_single_contact_at_the_ends(S, exe, tmp, Wc):
    """a candidate whose only contact is at the last waypoint (i = W, in a later pass) and one whose
    only contact is at i = 0 must be infeasible: the pass loop and the early exit.  The crafted arm's
    tool touches the floor only at drop >= 0.46; the paths hold it up everywhere but at one end."""
    world, r = TH.crafted_world()
    xml = H.write_xml(tmp, "crafted", W.mjcf(world))
    ch = S.Chain(S.Model(xml, joints=True), 3, count_static=False)
    n, degree = 6, 3
    up, down = np.array([0.0, 0.1, 0.0]), np.array([0.0, 0.47, 0.0])
    knots, flat = linear_ctrl(S, up, up, n, degree)
    last, first, free = flat.copy(), flat.copy(), flat.copy()
    last[-1], first[0] = down, down  # a clamped spline passes through its end control points
    ctrl = np.stack([free, last, first, free])
    want_feas, hits = host_feasible(S, exe, tmp, xml, 3, knots, degree, ctrl, Wc, "ends%d" % Wc)
    assert hits[1].tolist() == [0] * Wc + [1] and hits[2].tolist() == [1] + [0] * Wc and not hits[0].any()
    arc, feas, best = run_score(S, ch, knots, degree, ctrl, Wc)
    assert feas.tolist() == [True, False, False, True] == want_feas.tolist()
    check_scores(arc, feas, best, want_feas, job_arcs(S, knots, degree, ctrl, Wc))
    assert best[1] == 0  # two equal arcs: the lowest id


@pytest.mark.parametrize("B", [255, 256, 257, 513])
def test_score_ctrl_argmin_across_the_reduction(S, exe, tmp, B):
    """the single-query argmin at batches around and past its 256 threads (a thread then holds more
    than one candidate, and the tree reduces every slot), with ids past 2^32.  The crafted arm's
    `free` spline is feasible and `first` is not, so feasibility is placed candidate by candidate:
    (a) only the last candidate feasible; (b) two feasible candidates with identical splines 256
    apart, in one thread's stride: the lower id wins (batches of at least 257; a smaller one has
    no such pair); (c) none feasible: the record is {+inf, -1, 0}."""
    world, r = TH.crafted_world()
    xml = H.write_xml(tmp, "crafted", W.mjcf(world))
    ch = S.Chain(S.Model(xml, joints=True), 3, count_static=False)
    n, degree, Wc, first_id = 6, 3, 8, 2**40 + 5
    up, down = np.array([0.0, 0.1, 0.0]), np.array([0.0, 0.47, 0.0])
    knots, free = linear_ctrl(S, up, up, n, degree)
    first = free.copy()
    first[0] = down
    pair_feas, _ = host_feasible(S, exe, tmp, xml, 3, knots, degree, np.stack([free, first]), Wc, "argmin")
    assert pair_feas.tolist() == [True, False]
    cases = {"a": [B - 1], "c": []}
    if B >= 257:
        k = (B - 257) // 2
        cases["b"] = [k, k + 256]
    for name, feasible_at in cases.items():
        want_feas = np.zeros(B, bool)
        want_feas[feasible_at] = True
        ctrl = np.where(want_feas[:, None, None], free[None], first[None])
        arc, feas, best = run_score(S, ch, knots, degree, ctrl, Wc, first_id=first_id)
        check_scores(arc, feas, best, want_feas, job_arcs(S, knots, degree, ctrl, Wc), first_id)
        if name == "c":
            assert best[2] == 0 and best[1] == -1 and np.isposinf(best[0])
        else:
            assert best[1] == first_id + feasible_at[0]


# ------------------------------------------------------------------ sample_score
def test_sample_score(S, exe, tmp, arms):
    import torch
    from sspp_amd import _lib
    a = arms("arm7")
    D, n, degree, Wc, B, first_id, seed, sigma = 7, 8, 3, 40, 130, 11, 0xBEEF, 0.1
    ch = S.Chain(a["model"], D, count_static=False)
    start, end, _ = free_poses(exe, tmp, a["xml"], D)
    knots, c0 = linear_ctrl(S, start, end, n, degree)
    limits = np.full(D, np.pi)
    arc = torch.zeros(B, dtype=torch.float64, device="cuda")
    feas = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ctrl = torch.zeros((B, n, D), dtype=torch.float64, device="cuda")
    best = S.best_tensor()
    ch.sample_score(knots, degree, c0, sigma, limits, Wc, first_id, B, arc, feas, best, ctrl_out=ctrl, seed=seed)
    torch.cuda.synchronize()
    want = np.zeros((B, n, D))
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    c0c = np.ascontiguousarray(c0)
    _lib.check(_lib.lib().sspp_sample_ctrl_host(dp(knots), degree, dp(c0c), n, D, sigma, dp(limits), seed, first_id, B,
                                                dp(want)), "sample")
    got = _np(ctrl)
    assert got.tobytes() == want.tobytes()
    arc2, feas2, best2 = run_score(S, ch, knots, degree, want, Wc, first_id=first_id)
    assert _np(arc).tobytes() == arc2.tobytes() and np.array_equal(_np(feas).astype(bool), feas2)
    assert S.decode_best(best) == best2
    assert feas2.any() and not feas2.all()
    # without ctrl_out the chain keeps the candidates itself: the same results
    arc3 = torch.zeros(B, dtype=torch.float64, device="cuda")
    feas3 = torch.zeros(B, dtype=torch.uint8, device="cuda")
    best3 = S.best_tensor()
    ch.sample_score(knots, degree, c0, sigma, limits, Wc, first_id, B, arc3, feas3, best3, seed=seed)
    torch.cuda.synchronize()
    assert _np(arc3).tobytes() == arc2.tobytes() and S.decode_best(best3) == best2


# ------------------------------------------------------------------ count_static
def test_count_static(S, exe, tmp, arms):
    world = arm_world(3, 21)
    # two static boxes that overlap: one on the world, one on a body whose hinge (qpos address 3)
    # lies past the 3 driven values, so the body is static and the pair is evaluated once
    world["geoms"].append(dict(name="sa", type=W.BOX, size=(0.1, 0.1, 0.1), pos=(3, 3, 0.5)))
    world["bodies"].append(dict(name="gate", pos=(3.15, 3, 0.5), joints=[dict(type="hinge", axis=(0, 0, 1))],
                                geoms=[dict(name="sb", type=W.BOX, size=(0.1, 0.1, 0.1))]))
    model = S.Model(H.write_xml(tmp, "static", W.mjcf(world)), joints=True)
    knots, ctrl = random_splines(S, exe, tmp, arms("arm3")["xml"], 3, 40, 5, 3, 9)
    on, off = S.Chain(model, 3, count_static=True), S.Chain(model, 3, count_static=False)
    i = on.info()
    assert i["static_contacts"] > 0 and i["n_static_pairs"] > 0 and i["n_driven_bodies"] == 3
    arc1, feas1, best1 = run_score(S, on, knots, 3, ctrl, 30)
    assert not feas1.any() and np.all(np.isposinf(arc1)) and best1[1] == -1 and best1[2] == 0
    import torch
    assert _np(on.contacts(torch.zeros((5, 3), dtype=torch.float64, device="cuda"))).all()
    arc0, feas0, best0 = run_score(S, off, knots, 3, ctrl, 30)
    base = S.Chain(arms("arm3")["model"], 3, count_static=True)  # the world without the two boxes
    arc, feas, best = run_score(S, base, knots, 3, ctrl, 30)
    assert feas0.any() and np.array_equal(feas0, feas) and arc0.tobytes() == arc.tobytes() and best0 == best


# ------------------------------------------------------------------ limits
def star_world(n_links, n_balls=0):
    """n_links one-hinge links side by side on the world (and n_balls static spheres far away)"""
    bodies = [dict(name="s%d" % i, pos=(0.5 * i, 0, 1.0), joints=[dict(type="hinge", axis=(0, 1, 0))],
                   geoms=[dict(name="sg%d" % i, type=W.SPHERE, size=(0.05, 0, 0), pos=(0, 0, 0.2))]) for i in range(n_links)]
    balls = [dict(name="ball%d" % i, type=W.SPHERE, size=(0.01, 0, 0), pos=(0.1 * i, 5, 0.5)) for i in range(n_balls)]
    return dict(geoms=balls, bodies=bodies)


def test_limits(S, tmp):
    import torch
    from sspp_amd import _lib
    # driven bodies: a chain of 17 links under one driven joint
    for nj, ok in ((_lib.CHAIN_MAX_BODIES, True), (_lib.CHAIN_MAX_BODIES + 1, False)):
        m = S.Model(H.write_xml(tmp, "chain%d" % nj, W.mjcf(W.strip(W.random_arm(nj, 1, W.CAPSULE)))), joints=True)
        if ok:
            ch = S.Chain(m, 1)
            assert ch.info()["n_driven_bodies"] == nj
            gpos, _ = ch.fk(torch.zeros((3, 1), dtype=torch.float64, device="cuda"))
            assert np.isfinite(_np(gpos)).all()
        else:
            with pytest.raises(S.SsppError, match=r"\(-5\).*driven bodies"):
                S.Chain(m, 1)
    # dof: 9 scalar joints behind a free base is the largest pose
    m = S.Model(H.write_xml(tmp, "dof16", W.mjcf(W.strip(W.random_arm(10, 2, W.CAPSULE, free_base=True)))), joints=True)
    ch = S.Chain(m, _lib.CHAIN_MAX_DOF)
    assert ch.info()["n_driven_bodies"] == 11
    q = torch.as_tensor(W.arm_poses(16, 70, 1, 1.0, True), device="cuda")
    assert _np(ch.contacts(q)).shape == (70,)
    with pytest.raises(S.SsppError, match=r"\(-5\).*dof"):
        S.Chain(m, _lib.CHAIN_MAX_DOF + 1)
    with pytest.raises(S.SsppError, match=r"\(-1\).*nq"):
        S.Chain(S.Model(H.write_xml(tmp, "dof3", W.mjcf(star_world(3))), joints=True), 4)
    # pairs: one link against 512 balls fills the table, a 513th ball is one too many
    for balls, ok in ((_lib.CHAIN_MAX_PAIRS, True), (_lib.CHAIN_MAX_PAIRS + 1, False)):
        m = S.Model(H.write_xml(tmp, "pairs%d" % balls, W.mjcf(star_world(1, balls))), joints=True)
        if ok:
            ch = S.Chain(m, 1, count_static=False)
            assert ch.info()["n_pairs"] == balls == _lib.CHAIN_MAX_PAIRS
            assert not _np(ch.contacts(torch.zeros((65, 1), dtype=torch.float64, device="cuda"))).any()
        else:
            with pytest.raises(S.SsppError, match=r"\(-5\).*pairs"):
                S.Chain(m, 1)


# ------------------------------------------------------------------ the drop-in planner of an arm
def test_dropin_arm(S, exe, tmp, arms):
    from sspp import _sspp
    a = arms("arm7")
    D, sigma, samples, checks, n = 7, 0.08, 100, 100, 7
    pl = _sspp.SamplingPathPlanner7(a["xml"])
    start, end, touching = free_poses(exe, tmp, a["xml"], D)
    limits = np.pi * np.ones(D)
    found, paths = pl.plan(start, end, sigma, limits, samples, checks, n)
    # the same candidates through the chain
    sp = _sspp.Spline7()
    assert pl.initializePath(start, end, sp, n)
    knots, c0 = np.array(sp.knots()), np.ascontiguousarray(np.array(sp.ctrls()).T)
    cand = np.array([np.array(pl.sampleWithNoise(sp, sigma, limits, k).ctrls()).T for k in range(samples)])
    ch = S.Chain(a["model"], D, count_static=True)
    arc, feas, best = run_score(S, ch, knots, 3, np.ascontiguousarray(cand), checks)
    want_feas, _ = host_feasible(S, exe, tmp, a["xml"], D, knots, 3, cand, checks, "dropin")
    np.testing.assert_array_equal(feas, want_feas)
    assert 0 < feas.sum() < samples, feas.sum()
    assert found and list(pl.last_feasible_ids) == list(np.flatnonzero(feas)) and len(paths) == feas.sum()
    for s, k in zip(paths, np.flatnonzero(feas)):
        assert np.array(s.ctrls()).T.tobytes() == cand[k].tobytes()
    assert pl.last_best_index == best[1] == int(np.flatnonzero(feas)[np.argmin(arc[feas])]) and pl.last_best_cost == best[0]
    assert np.array(pl.get_ctrl_pts()).T.tobytes() == cand[best[1]].tobytes()
    assert pl.evaluate(0.0).tobytes() == paths[list(pl.last_feasible_ids).index(best[1])](0.0).tobytes()
    for s in paths[:10]:
        assert pl.checkCollision(s, checks) is False
    bad = _sspp.Spline7()
    pl.initializePath(start, touching, bad, n)
    assert pl.checkCollision(bad, checks) is True
    assert pl.computeArcLength(paths[0], checks) == arc[np.flatnonzero(feas)[0]]
    out = _sspp.Spline7()
    assert pl.findBestPath(paths, out, checks) and np.array(out.ctrls()).tobytes() == np.array(pl.get_ctrl_pts()).tobytes()
    for call in (lambda: pl.plan_many(start[None], end[None], sigma, limits, samples, checks, n),
                 lambda: pl.set_qpos(np.zeros(7)), lambda: pl.get_qpos(),
                 lambda: pl.set_body_pose("link0", np.zeros(3), np.array([1.0, 0, 0, 0])),
                 lambda: pl.contact_report(paths[0], checks)):
        with pytest.raises(RuntimeError, match="(?i)unsupported"):
            call()


def test_dropin_free_body_file_unchanged(S):
    """scenes/robocrane.xml through the drop-in (now the joint-accepting loader): the planner takes
    the scene / planner objects, and plan() returns what the C ABI's free-body path returns"""
    from sspp import _sspp
    path = os.path.join(S.SCENE_DIR, "robocrane.xml")
    pl = _sspp.SamplingPathPlanner7(path)
    start = np.array([0.5, 0.15, 0.136, 0.707, 0, 0, 0.707])
    end = np.array([0.5, -0.05, 0.136, 0.707, 0, 0, 0.707])
    found, paths = pl.plan(start, end, 0.08, np.ones(7), 64, 50, 10)
    assert pl._option(11) > 0  # (SSPP_OPT_NPAIRS: a job of the free-body path ran)
    assert len(pl.get_qpos()) > 7
    from sspp_amd import _lib
    knots, ctrl, feas, arc, best = np.zeros(14), np.zeros((64, 10, 7)), np.zeros(64, np.uint8), np.zeros(64), _lib.Best()
    scene = S.Scene(S.Model(path), 0, 7)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    lim = np.ones(7)
    _lib.check(_lib.lib().sspp_plan_sspp(scene.handle, 7, dp(start), dp(end), 0.08, dp(lim), 64, 50, 10, pl.seed, dp(knots),
                                         dp(ctrl), feas.ctypes.data_as(C.POINTER(C.c_uint8)), dp(arc), C.byref(best)), "plan")
    assert list(pl.last_feasible_ids) == list(np.flatnonzero(feas)) and pl.last_best_index == best.index
    assert pl.last_best_cost == best.cost and found == (best.index >= 0)
