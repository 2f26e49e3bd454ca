"""Worlds for arms on the GPU: Chain.set_qpos / set_body_pose / get_qpos / epoch, and a world per query
(Chain.sample_score_queries / plan_many with worlds=).

After an update every chain call is compared byte for byte with the stand-alone host program in the
new world (tests/chain_world/check_world.cpp runs the same __host__ __device__ routines on tables
built by the same builder; it is checked against tests/chain_world_ref.py in
tests/test_chain_world_host.py), with a fresh Chain from a rewritten MJCF where a file expresses the
world, and with a Chain of dof = nq fed the world's values as pose values.  Row q of a worlds launch
is compared byte for byte with Chain.sample_score after set_qpos(worlds[q]) on a second chain; what
the sets hold (a pair of queries that differ in their world alone and decide differently, mixed
queries, a world with static contacts between two without) is asserted from the host program's
decisions before anything is compared with the device.
"""
import gc

import numpy as np
import pytest

from tests import chain_host as H
from tests import chain_query_cases as QC
from tests import chain_ref as R
from tests import chain_report_host as CRH
from tests import chain_scenes as W
from tests import chain_world_host as WH
from tests import chain_world_scenes as WS
from tests import test_gpu_chain as G
from tests import test_gpu_chain_queries as GQ
from tests.test_gpu_chain import S  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

BIG_ID = 2 ** 40 + 5
E_INVAL = r"\(-1\)"
# The cell is planned with dof = 5 where no spline is scored (fk, contacts, the pose report).  The
# scene-less job behind every scoring call is instantiated for dof 1, 2, 3, 4, 6, 7 and 9 only, so the
# scoring calls plan the same cell with dof = 4: joints 4, 5 (the slide with ref != 0) and 6 are then
# frozen joints on driven bodies.
D, D_POSES, DEG = 4, 5, 3
MIXED_SIGMAS = (0.1, 0.05, 0.2, 0.3, 0.5, 0.02, 0.8)  # tried in this order until the host program finds the query mixed
MIN_EACH = 2


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def exe(cuda, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chain_world_gpu") / "check_world")
    r = WH.build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("chain_world_gpu_files")


@pytest.fixture(scope="module")
def cell(S, tmp):
    c = WS.cell()
    c["xml"] = H.write_xml(tmp, "cell", W.mjcf(c["world"]))
    c["m"] = R.flatten(c["world"])
    c["names"] = c["m"]["body_names"]
    c["model"] = S.Model(c["xml"], joints=True)
    c["qpos0"] = c["model"].arrays()["qpos0"].copy()
    c["worlds"] = WS.cell_worlds(c["qpos0"])
    c["worlds"].append(dict(qpos=c["worlds"][1]["qpos"], poses=c["worlds"][3]["poses"][:3]))  # (undone exactly: see undo)
    return c


def apply(ch, world):
    if world["qpos"] is not None:
        ch.set_qpos(world["qpos"])
    for name, pos, quat in world["poses"]:
        ch.set_body_pose(name, pos, quat)
    return (world["qpos"] is not None) + len(world["poses"])


def undo(ch, c, world):
    """back to the model's own world: its qpos0, and the re-posed bodies' own poses.  Those bodies'
    own quaternions are exactly (1, 0, 0, 0), which the normalisation of an update returns as it is."""
    arrs = c["model"].arrays()
    n = 0
    for name, _, _ in world["poses"]:
        b = c["names"].index(name)
        assert tuple(arrs["body_quat"][b]) == (1.0, 0.0, 0.0, 0.0)
        ch.set_body_pose(b, arrs["body_pos"][b], arrs["body_quat"][b])
        n += 1
    ch.set_qpos(c["qpos0"])
    return n + 1


def host(exe, tmp, c, world, q, tag, count_static=0, dof=D):
    o = WH.run(exe, c["xml"], dof, WH.world_ops(c["names"], world), q, tmp, count_static=count_static, tag=tag)
    assert o["rc"] == 0 and all(x[0] == 0 for x in o["ops"]), (o["err"], o["ops"])
    return o


def waypoints(S, knots, ctrl, Wc):
    return np.array([[S.spline_eval(knots, DEG, ctrl[b], i / Wc) for i in range(Wc + 1)] for b in range(len(ctrl))])


def host_paths(S, exe, tmp, c, world, knots, ctrl, Wc, tag, count_static=0):
    """the host program over every waypoint of the splines: (feasible [B] bool, first [B, 2], its output)"""
    B = len(ctrl)
    o = host(exe, tmp, c, world, waypoints(S, knots, ctrl, Wc).reshape(-1, D), tag, count_static)
    P = o["info"]["n_pairs"]
    return ~o["hit"].reshape(B, Wc + 1).astype(bool).any(1), CRH.path_first(o["contact"].reshape(B, Wc + 1, P)), o


LINE_POINTS = 200  # a free pair is kept when the straight line between its poses is free on this grid


def free_pair(exe, tmp, c, world, seed=77):
    """two nearby poses that the host program finds free in the world, the straight line between
    them (a query's initial spline) free too, and a touching pose; pools tried from `seed` on"""
    t = np.linspace(0.0, 1.0, LINE_POINTS + 1)[:, None]
    for s in range(seed, seed + 8):
        pool = W.arm_poses(D, 400, s, 1.2)
        hit = host(exe, tmp, c, world, pool, "pool")["hit"].astype(bool)
        free = pool[~hit]
        if len(free) < 8 or not hit.any():
            continue
        for e in np.argsort(np.abs(free - free[0]).max(1))[1:9]:
            if not host(exe, tmp, c, world, (1 - t) * free[0] + t * free[e], "line")["hit"].any():
                return free[0], free[e], pool[hit][0]
    raise AssertionError("no free path in the pools")


def device_outputs(S, ch, q, knots, ctrl, Wc, init, sigma, seed, first_id):
    """every call of the list on one chain, as bytes-comparable arrays"""
    import torch
    out = {}
    dq = torch.as_tensor(q, device="cuda")
    for N in (1, 65):
        gpos, gmat = ch.fk(dq[:N])
        out["fk%d" % N] = np.concatenate([_np(gpos), _np(gmat)], 2)
        out["hit%d" % N] = _np(ch.contacts(dq[:N]))
        pc, pd = ch.pair_contacts(dq[:N])
        out["pc%d" % N], out["pd%d" % N] = _np(pc), _np(pd)
    dctrl = torch.as_tensor(np.ascontiguousarray(ctrl), device="cuda")
    out["first"] = _np(ch.first_contacts(knots, DEG, dctrl, Wc))
    arc, feas, best = G.run_score(S, ch, knots, DEG, ctrl, Wc, first_id)
    out["score_arc"], out["score_feas"], out["score_best"] = arc, feas, np.array(best)
    B, n = ctrl.shape[:2]
    qs = dict(knots=knots, init=init[None], sigma=np.array([sigma]), limits=np.full((1, D), np.pi), seeds=np.array([seed]))
    one = GQ.run_single(S, ch, qs, 0, DEG, Wc, first_id, B)
    for k, v in one.items():
        out["sample_" + k] = v
    return out


# ------------------------------------------------------------------ 1. re-posing: the host program's bytes
# world, B, W: every N, B and W of the issue (N in device_outputs)
REPOSE_CASES = [(1, 1, 40), (2, 63, 64), (3, 65, 65), (4, 65, 40)]


@pytest.mark.parametrize("k,B,Wc", REPOSE_CASES)
def test_repose_equals_host_bytes(S, exe, tmp, cell, k, B, Wc):
    c, world, n = cell, cell["worlds"][k], 8
    ch = S.Chain(c["model"], D, count_static=False)
    q = WS.cell_poses(D, 65, 40 + k)
    start, end, _ = free_pair(exe, tmp, c, world)
    knots, init = G.linear_ctrl(S, start, end, n, DEG)
    rng = np.random.default_rng(k)
    ctrl = np.ascontiguousarray(init[None] + rng.normal(0.0, 0.25, (B, n, D)) * rng.uniform(0.0, 2.0, (B, 1, 1)))
    args = (q, knots, ctrl, Wc, init, 0.2, 0xC0FFEE + k, BIG_ID if k % 2 else 0)
    first = device_outputs(S, ch, *args)
    assert ch.epoch == 0
    np.testing.assert_array_equal(ch.get_qpos(), c["qpos0"])
    calls = apply(ch, world)
    assert ch.epoch == calls
    np.testing.assert_array_equal(ch.get_qpos(), WS.norm_world(world["qpos"], c["free"]))
    got = device_outputs(S, ch, *args)
    # the host program in the new world
    o = host(exe, tmp, c, world, q, "poses")
    assert ch.info() == dict(o["info"], dof=D)
    assert [(p["geom1"], p["geom2"], int(p["moving1"]), int(p["moving2"]), p["margin"]) for p in ch.pairs()] == o["pairs"]
    assert [(p["geom1"], p["geom2"], p["margin"], p["contact"], p["deep"]) for p in ch.static_pairs()] == o["statics"]
    for N in (1, 65):
        assert got["fk%d" % N].tobytes() == o["fk"][:N].tobytes(), (N, np.abs(got["fk%d" % N] - o["fk"][:N]).max())
        assert got["hit%d" % N].tobytes() == o["hit"][:N].tobytes()
        assert got["pc%d" % N].tobytes() == o["contact"][:N].tobytes() and got["pd%d" % N].tobytes() == o["deep"][:N].tobytes()
    assert got["fk65"].tobytes() != first["fk65"].tobytes()
    feas, path_first, _ = host_paths(S, exe, tmp, c, world, knots, ctrl, Wc, "paths")
    assert got["first"].tobytes() == path_first.tobytes()
    first_id = args[-1]
    G.check_scores(got["score_arc"], got["score_feas"], tuple(got["score_best"]), feas, G.job_arcs(S, knots, DEG, ctrl, Wc),
                   first_id)
    sfeas, _, _ = host_paths(S, exe, tmp, c, world, knots, got["sample_ctrl"], Wc, "sampled")
    rec = got["sample_best"]
    best = (float(rec[:1].view(np.float64)[0]), int(rec[1]), int(rec[2]))
    G.check_scores(got["sample_arc"], got["sample_feasible"].astype(bool), best, sfeas,
                   G.job_arcs(S, knots, DEG, got["sample_ctrl"], Wc), first_id)
    assert got["sample_ctrl"].tobytes() == first["sample_ctrl"].tobytes()  # (the sampler does not see the world)
    print("world", k, "score feasible %d of %d, sampled feasible %d of %d" % (feas.sum(), B, sfeas.sum(), B))
    if not any(name == "link6" for name, _, _ in world["poses"]):  # back in the first world: the first outputs again
        undo(ch, c, world)
        again = device_outputs(S, ch, *args)
        for key in first:
            assert again[key].tobytes() == first[key].tobytes(), key


@pytest.mark.parametrize("k", [1, 2, 3])
def test_repose_dof5_poses_equal_host_bytes(S, exe, tmp, cell, k):
    """the issue's dof = 5 (joints 5 and 6 frozen): the per-pose calls in the new world and back"""
    import torch
    c, world = cell, cell["worlds"][k]
    ch = S.Chain(c["model"], D_POSES, count_static=False)
    q = WS.cell_poses(D_POSES, 65, 60 + k)
    dq = torch.as_tensor(q, device="cuda")
    first = _np(ch.fk(dq)[0])
    apply(ch, world)
    o = host(exe, tmp, c, world, q, "poses5", dof=D_POSES)
    assert ch.info() == dict(o["info"], dof=D_POSES)
    for N in (1, 65):
        gpos, gmat = ch.fk(dq[:N])
        assert np.concatenate([_np(gpos), _np(gmat)], 2).tobytes() == o["fk"][:N].tobytes(), N
        assert _np(ch.contacts(dq[:N])).tobytes() == o["hit"][:N].tobytes()
        pc, pd = ch.pair_contacts(dq[:N])
        assert _np(pc).tobytes() == o["contact"][:N].tobytes() and _np(pd).tobytes() == o["deep"][:N].tobytes()
    assert 0 < o["hit"].sum() < 65
    if k != 3:
        ch.set_qpos(c["qpos0"])
        assert _np(ch.fk(dq)[0]).tobytes() == first.tobytes()


def test_repose_equals_fresh_chain(S, exe, tmp, cell):
    """a world that an MJCF expresses (a free body's pose, body poses): a fresh Chain from the file"""
    c = cell
    poses = [("block", WS.BLOCK_UP, [0.9, 0.1, -0.3, 0.2])] + c["worlds"][3]["poses"]
    world = dict(qpos=None, poses=poses)
    xml2 = H.write_xml(tmp, "cell_rewritten", W.mjcf(WS.with_world(c["world"], {n: (p, qt) for n, p, qt in poses})))
    fresh = S.Chain(S.Model(xml2, joints=True), D, count_static=True)
    ch = S.Chain(c["model"], D, count_static=True)
    assert ch.info()["static_contacts"] > 0  # (the block rests on the floor; the update lifts it)
    apply(ch, world)
    assert ch.info() == fresh.info() and ch.info()["static_contacts"] == 0
    assert ch.static_pairs() == fresh.static_pairs()
    np.testing.assert_array_equal(ch.get_qpos(), fresh.get_qpos())
    start, end, _ = free_pair(exe, tmp, c, world)
    knots, init = G.linear_ctrl(S, start, end, 4, DEG)
    ctrl = np.ascontiguousarray(init[None] + np.random.default_rng(5).normal(0.0, 0.3, (63, 4, D)))
    args = (WS.cell_poses(D, 65, 44), knots, ctrl, 40, init, 0.2, 0xFACE, 0)
    a, b = device_outputs(S, ch, *args), device_outputs(S, fresh, *args)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert 0 < a["sample_feasible"].sum() + a["score_feas"].sum()


@pytest.mark.parametrize("k,dof", [(1, 5), (2, 4)])
def test_fk_equals_full_dof_chain(S, cell, k, dof):
    """Chain(model, D).fk(q) in world w equals Chain(model, nq).fk(concat(q, w[D:])): host and device
    run the same written-out operations, so bytes are expected and asserted."""
    c = cell
    assert c["nq"] <= 16
    ch, full = S.Chain(c["model"], dof, count_static=False), S.Chain(c["model"], c["nq"], count_static=False)
    ch.set_qpos(c["worlds"][k]["qpos"])
    w = ch.get_qpos()
    q = WS.cell_poses(dof, 65, 50 + k)
    gp, gm = ch.fk(q)
    fp, fm = full.fk(np.concatenate([q, np.tile(w[dof:], (len(q), 1))], 1))
    print("max |difference|", float((gp - fp).abs().max()), float((gm - fm).abs().max()))
    assert _np(gp).tobytes() == _np(fp).tobytes() and _np(gm).tobytes() == _np(fm).tobytes()


def test_update_loop_keeps_resources(S, exe, tmp, cell):
    c = cell
    ch = S.Chain(c["model"], D, count_static=False)
    start, end, _ = free_pair(exe, tmp, c, c["worlds"][0])
    limits = np.full(D, np.pi)
    plan = lambda: GQ.plan_host(S, ch, start, end, limits, 7, 0.1, 65, 40, 8)  # noqa: E731
    apply(ch, c["worlds"][4])
    first = plan()
    gc.collect()
    before = GQ.live(S)
    bests = []
    for i in range(20):
        apply(ch, c["worlds"][1 + i % 2])
        bests.append(plan()["best"])
        assert GQ.live(S) == before, i
    assert ch.epoch == 4 + 20 and all(b == bests[i % 2] for i, b in enumerate(bests))
    undo(ch, c, c["worlds"][4])
    apply(ch, c["worlds"][4])
    assert plan()["best"] == first["best"]


# ------------------------------------------------------------------ 2. a world per query
def world_rows(c, Q):
    """Q worlds' qpos: the cell's three qpos worlds in turn, the block moved a little more each round"""
    base = [c["qpos0"], c["worlds"][1]["qpos"], c["worlds"][2]["qpos"]]
    out = []
    for q in range(Q):
        w = np.array(base[q % 3], float)
        w[c["block"] + 1] += 0.01 * (q // 3)
        w[4] += 0.05 * (q % 4)  # (joint 4: frozen at dof = 4)
        w[c["door"]] += 0.02 * (q // 3)
        out.append(w)
    return np.ascontiguousarray(np.array(out))


def query_set(S, exe, tmp, c, Q, n, sigmas=(0.1, 0.2, 0.05, 0.3)):
    start, end, touching = free_pair(exe, tmp, c, c["worlds"][0])
    init, sigma, limits, seeds = [], [], [], []
    knots = None
    for q in range(Q):
        s, e = (start, end) if q % 4 != 3 else (end, start)
        knots, c0 = G.linear_ctrl(S, s, e, n, DEG)
        init.append(c0)
        sigma.append(sigmas[q % len(sigmas)])
        limits.append(np.full(D, np.pi) * (1.0 - 0.004 * q))
        seeds.append(0xBEEF + 1000003 * q)
    return dict(knots=knots, init=np.ascontiguousarray(np.array(init)), sigma=np.array(sigma),
                limits=np.ascontiguousarray(np.array(limits)), seeds=np.array(seeds, dtype=np.uint64), kinds=["q"] * Q)


def run_worlds(S, ch, qs, worlds, Wc, first_id, B, null=()):
    """one worlds launch into sentinel-filled buffers; `null`: the outputs passed as None"""
    import torch
    Q, n, _ = qs["init"].shape
    arc = torch.full((Q, B), -1.0, dtype=torch.float64, device="cuda")
    feas = torch.full((Q, B), 7, dtype=torch.uint8, device="cuda")
    ctrl = None if "ctrl" in null else torch.full((Q, B, n, D), -2.0, dtype=torch.float64, device="cuda")
    best = None if "best" in null else torch.full((Q, 4), -3, dtype=torch.int64, device="cuda")
    bctrl = None if "best_ctrl" in null else torch.full((Q, n, D), -4.0, dtype=torch.float64, device="cuda")
    ch.sample_score_queries(qs["knots"], DEG, qs["init"], qs["sigma"], qs["limits"], qs["seeds"], Wc, first_id, B, arc,
                            feas, best=best, ctrl_out=ctrl, best_ctrl=bctrl, worlds=worlds)
    torch.cuda.synchronize()
    return dict(arc=_np(arc), feasible=_np(feas), ctrl=_np(ctrl), best=_np(best), best_ctrl=_np(bctrl))


def assert_rows_equal_loop(S, got, loop, qs, worlds, Wc, first_id, B):
    """row q against set_qpos(worlds[q]) + Chain.sample_score on the chain `loop`"""
    singles = []
    for q in range(len(worlds)):
        loop.set_qpos(worlds[q])
        one = GQ.run_single(S, loop, qs, q, DEG, Wc, first_id, B)
        singles.append(one)
        assert got["arc"][q].tobytes() == one["arc"].tobytes(), q
        assert got["feasible"][q].tobytes() == one["feasible"].tobytes(), q
        assert set(np.unique(one["feasible"])) <= {0, 1}
        if got["ctrl"] is not None:
            assert got["ctrl"][q].tobytes() == one["ctrl"].tobytes(), q
        if got["best"] is not None:
            assert got["best"][q].tobytes() == one["best"].tobytes(), (q, got["best"][q], one["best"])
        if got["best_ctrl"] is not None:
            assert got["best_ctrl"][q].tobytes() == GQ.winner_row(one, first_id).tobytes(), q
    return singles


# Q, B, W, n, first id, outputs passed as null: every Q, B, W, n and first id of the issue (no query
# boundary on a multiple of 64), each nullable output null in turn
WORLD_CASES = [(1, 1, 40, 4, 0, ()), (2, 63, 65, 8, BIG_ID, ("ctrl",)), (5, 65, 40, 4, 0, ("best",)),
               (64, 130, 65, 8, BIG_ID, ("best_ctrl",)), (5, 130, 40, 8, 0, ()), (64, 1, 40, 4, BIG_ID, ("ctrl", "best"))]


@pytest.mark.parametrize("Q,B,Wc,n,first_id,null", WORLD_CASES)
def test_world_rows_equal_set_qpos_loop(S, exe, tmp, cell, Q, B, Wc, n, first_id, null):
    c = cell
    ch, loop = S.Chain(c["model"], D, count_static=False), S.Chain(c["model"], D, count_static=False)
    qs, worlds = query_set(S, exe, tmp, c, Q, n), world_rows(c, Q)
    got = run_worlds(S, ch, qs, worlds, Wc, first_id, B, null)
    assert_rows_equal_loop(S, got, loop, qs, worlds, Wc, first_id, B)
    assert ch.epoch == 0
    np.testing.assert_array_equal(ch.get_qpos(), c["qpos0"])
    print("feasible per query", got["feasible"].sum(1).tolist())
    if Q * B >= 64 * 130:
        assert got["feasible"].any() and not got["feasible"].all()


def test_world_rows_after_body_poses(S, exe, tmp, cell):
    """body poses are the chain's: a worlds launch on a chain whose bodies were re-posed"""
    c = cell
    ch, loop = S.Chain(c["model"], D, count_static=False), S.Chain(c["model"], D, count_static=False)
    for x in (ch, loop):
        apply(x, dict(qpos=None, poses=c["worlds"][3]["poses"]))
    qs, worlds = query_set(S, exe, tmp, c, 5, 8), world_rows(c, 5)
    got = run_worlds(S, ch, qs, worlds, 40, 3, 63)
    assert_rows_equal_loop(S, got, loop, qs, worlds, 40, 3, 63)
    assert ch.epoch == 4


def test_world_set_properties(S, exe, tmp, cell):
    """what the set holds, from the host program alone: queries 0 and 1 are identical but for their
    world (the block far away / the block on the start pose's tool) and decide differently; queries
    0, 2 and 3 are mixed"""
    c = cell
    B, Wc, n, first_id = 65, 40, 8, 11
    names = c["names"]
    far = np.array(c["worlds"][1]["qpos"], float)
    start, end, _ = free_pair(exe, tmp, c, dict(qpos=far, poses=[]))
    tool = c["model"].geom_id("tool")
    at_tool = far.copy()
    at_tool[c["block"]:c["block"] + 3] = host(exe, tmp, c, dict(qpos=far, poses=[]), start[None], "tool")["fk"][0, tool, :3]
    w2 = np.array(c["worlds"][2]["qpos"], float)
    s2, e2, _ = free_pair(exe, tmp, c, dict(qpos=w2, poses=[]), seed=78)
    worlds = np.ascontiguousarray(np.array([far, at_tool, w2, far]))
    ends = [(start, end), (start, end), (s2, e2), (end, start)]
    knots = G.linear_ctrl(S, start, end, n, DEG)[0]
    qs = dict(knots=knots, init=np.zeros((4, n, D)), sigma=np.zeros(4), limits=np.tile(np.full(D, np.pi), (4, 1)),
              seeds=np.array([0xD00D, 0xD00D, 0xD00D + 1, 0xD00D + 2], dtype=np.uint64), kinds=["q"] * 4)
    for q, (s, e) in enumerate(ends):
        qs["init"][q] = G.linear_ctrl(S, s, e, n, DEG)[1]
    want = [None] * 4
    for q in (0, 2, 3):  # a sigma at which the host program finds the query mixed
        for sg in MIXED_SIGMAS:
            qs["sigma"][q] = sg
            one = dict(qs, init=qs["init"][q:q + 1], sigma=qs["sigma"][q:q + 1], limits=qs["limits"][q:q + 1], seeds=qs["seeds"][q:q + 1])
            cand = QC.sampled(S, one, DEG, first_id, B)[0]
            f, _, _ = host_paths(S, exe, tmp, c, dict(qpos=worlds[q], poses=[]), knots, cand, Wc, "mix%d" % q)
            print("query", q, "sigma", sg, "feasible %d of %d" % (f.sum(), B))
            if MIN_EACH <= f.sum() <= B - MIN_EACH:
                want[q] = f
                break
        assert want[q] is not None, "no sigma of the list makes query %d mixed" % q
    qs["sigma"][1] = qs["sigma"][0]
    cand = QC.sampled(S, qs, DEG, first_id, B)
    assert cand[0].tobytes() == cand[1].tobytes()
    want[1] = host_paths(S, exe, tmp, c, dict(qpos=worlds[1], poses=[]), knots, cand[1], Wc, "blocked")[0]
    assert (want[0] != want[1]).any() and not want[1].any()
    ch, loop = S.Chain(c["model"], D, count_static=False), S.Chain(c["model"], D, count_static=False)
    got = run_worlds(S, ch, qs, worlds, Wc, first_id, B)
    assert got["ctrl"].tobytes() == cand.tobytes()
    for q in range(4):
        np.testing.assert_array_equal(got["feasible"][q].astype(bool), want[q])
        assert 0 < want[q].sum() < B or q == 1
    assert got["feasible"][0].tobytes() != got["feasible"][1].tobytes()
    assert_rows_equal_loop(S, got, loop, qs, worlds, Wc, first_id, B)


def test_world_static_contacts(S, exe, tmp, cell):
    """count_static = 1: the world with the block on the floor between two with it lifted"""
    c = cell
    up, up2 = c["qpos0"].copy(), c["qpos0"].copy()
    up[c["block"]:c["block"] + 3] = (3.5, 3.5, 2.0)  # (out of the arm's reach)
    up2[c["block"]:c["block"] + 3] = (3.5, -3.5, 2.0)
    worlds = np.ascontiguousarray(np.array([up, c["qpos0"], up2]))
    counts = [host(exe, tmp, c, dict(qpos=w, poses=[]), c["qpos0"][None, :D], "st%d" % i, 1)["info"]["static_contacts"]
              for i, w in enumerate(worlds)]
    assert counts[0] == 0 and counts[1] > 0 and counts[2] == 0
    ch, loop = S.Chain(c["model"], D, count_static=True), S.Chain(c["model"], D, count_static=True)
    qs = query_set(S, exe, tmp, c, 3, 8, sigmas=(0.05, 0.03, 0.04))
    got = run_worlds(S, ch, qs, worlds, 40, 0, 65)
    assert not got["feasible"][1].any() and np.all(np.isposinf(got["arc"][1])) and not got["best_ctrl"][1].any()
    assert got["best"][1][1] == -1 and got["best"][1][2] == 0
    assert got["feasible"][0].any() and got["feasible"][2].any()
    assert_rows_equal_loop(S, got, loop, qs, worlds, 40, 0, 65)
    off = run_worlds(S, S.Chain(c["model"], D, count_static=False), qs, worlds, 40, 0, 65)
    assert off["feasible"][1].any()  # (without count_static the same world blocks nothing)
    for q in (0, 2):
        assert off["arc"][q].tobytes() == got["arc"][q].tobytes()


def test_identical_worlds_equal_plain_queries(S, exe, tmp, cell):
    c = cell
    ch = S.Chain(c["model"], D, count_static=False)
    ch.set_qpos(c["worlds"][2]["qpos"])
    qs = query_set(S, exe, tmp, c, 5, 8)
    plain = GQ.run_queries(S, ch, qs, DEG, 65, BIG_ID, 63)
    got = run_worlds(S, ch, qs, np.tile(ch.get_qpos(), (5, 1)), 65, BIG_ID, 63)
    for k in plain:
        assert got[k].tobytes() == plain[k].tobytes(), k


def test_full_dof_arm_accepts_worlds(S, exe, tmp):
    """nq == dof: worlds are accepted and change nothing"""
    f = WS.full()
    model = S.Model(H.write_xml(tmp, "full", W.mjcf(f["world"])), joints=True)
    ch = S.Chain(model, 3, count_static=False)
    q = W.arm_poses(3, 65, 9, 2.0)
    before = _np(ch.fk(q)[0])
    ch.set_qpos([0.4, -0.3, 0.05])
    assert ch.epoch == 1 and _np(ch.fk(q)[0]).tobytes() == before.tobytes()
    knots, c0 = G.linear_ctrl(S, q[0], q[1], 4, DEG)
    qs = dict(knots=knots, init=np.ascontiguousarray(np.array([c0, c0])), sigma=np.array([0.2, 0.3]),
              limits=np.full((2, 3), np.pi), seeds=np.array([1, 2], dtype=np.uint64), kinds=["q"] * 2)
    import torch
    outs = []
    for worlds in (None, np.array([[0.1, 0.2, 0.0], [-1.0, 0.5, 0.1]])):
        arc = torch.full((2, 63), -1.0, dtype=torch.float64, device="cuda")
        feas = torch.full((2, 63), 7, dtype=torch.uint8, device="cuda")
        ch.sample_score_queries(knots, DEG, qs["init"], qs["sigma"], qs["limits"], qs["seeds"], 40, 0, 63, arc, feas, worlds=worlds)
        torch.cuda.synchronize()
        outs.append((_np(arc).tobytes(), _np(feas).tobytes()))
    assert outs[0] == outs[1]


# ------------------------------------------------------------------ 3. plan_many with worlds
@pytest.mark.parametrize("Q", [3, 65])
def test_plan_many_worlds(S, exe, tmp, cell, Q):
    c = cell
    ch, loop = S.Chain(c["model"], D, count_static=True), S.Chain(c["model"], D, count_static=True)
    start, end, touching = free_pair(exe, tmp, c, c["worlds"][1])
    starts = np.ascontiguousarray(np.array([start if q % 5 != 4 else touching for q in range(Q)]))
    ends = np.ascontiguousarray(np.array([end if q % 2 == 0 else start for q in range(Q)]))
    starts[1::2] = end
    worlds = np.tile(np.array(c["worlds"][1]["qpos"], float), (Q, 1))  # (start, end and their line are free in it)
    for q in range(Q):
        worlds[q, c["door"]] += 0.02 * q
        worlds[q, 6] += 0.01 * (q % 4)
        if q % 7 == 6:
            worlds[q] = c["worlds"][2]["qpos"]
    worlds[1] = c["qpos0"]  # the block on the floor: a static contact
    seeds = [0xA11CE + 17 * q for q in range(Q)]
    limits = np.full(D, np.pi)
    P = dict(sigma=0.1, sample_count=65, check_points=40, init_points=8)
    out = ch.plan_many(starts, ends, P["sigma"], limits, P["sample_count"], P["check_points"], P["init_points"], seeds=seeds,
                       return_all=True, worlds=worlds)
    assert ch.epoch == 0
    winners = 0
    for q in range(Q):
        loop.set_qpos(worlds[q])
        one = GQ.plan_host(S, loop, starts[q], ends[q], limits, seeds[q], **P)
        assert one["reserved"] == 0 and out["knots"].tobytes() == one["knots"].tobytes()
        assert np.array(out["best"][q][:1]).tobytes() == np.array(one["best"][:1]).tobytes() and out["best"][q][1:] == one["best"][1:]
        assert out["n_feasible"][q] == one["best"][2] == int(one["feasible"].sum())
        row = one["ctrl"][one["best"][1]] if one["best"][1] >= 0 else np.zeros_like(one["ctrl"][0])
        assert out["best_ctrl"][q].tobytes() == row.tobytes(), q
        assert out["arc"][q].tobytes() == one["arc"].tobytes() and out["feasible"][q].tobytes() == one["feasible"].tobytes()
        winners += one["best"][1] >= 0
    assert 0 < winners < Q
    assert out["best"][1][1] == -1  # (the block on the floor: static contacts block the query)


# ------------------------------------------------------------------ 4. state, resources, refusals
def test_state_and_resources(S, exe, tmp, cell):
    c = cell
    ch = S.Chain(c["model"], D, count_static=False)
    ch.set_qpos(c["worlds"][1]["qpos"])
    qs, worlds = query_set(S, exe, tmp, c, 5, 8), world_rows(c, 5)
    before = GQ.run_single(S, ch, qs, 0, DEG, 40, 0, 65)
    world_before, epoch_before = ch.get_qpos(), ch.epoch
    first = run_worlds(S, ch, qs, worlds, 40, 0, 65)
    gc.collect()
    live = GQ.live(S)
    for _ in range(3):
        again = run_worlds(S, ch, qs, worlds[::-1].copy(), 40, 0, 65)
        back = run_worlds(S, ch, qs, worlds, 40, 0, 65)
        assert GQ.live(S) == live
        assert back["arc"].tobytes() == first["arc"].tobytes() and back["best"].tobytes() == first["best"].tobytes()
        assert again["feasible"][2].tobytes() == first["feasible"][2].tobytes()  # (the middle query keeps its world)
    after = GQ.run_single(S, ch, qs, 0, DEG, 40, 0, 65)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    assert ch.epoch == epoch_before
    np.testing.assert_array_equal(ch.get_qpos(), world_before)
    plain = GQ.run_queries(S, ch, qs, DEG, 40, 0, 65)  # (the plain query call is as it was: the chain's own world)
    for q in range(5):
        one = GQ.run_single(S, ch, qs, q, DEG, 40, 0, 65)
        assert plain["arc"][q].tobytes() == one["arc"].tobytes() and plain["feasible"][q].tobytes() == one["feasible"].tobytes()
    del ch
    gc.collect()


def test_refusals(S, exe, tmp, cell):
    import torch
    c = cell
    ch = S.Chain(c["model"], D, count_static=False)
    big, n, B, Wc = query_set(S, exe, tmp, c, 65, 4), 4, 8, 40
    worlds = world_rows(c, 65)
    arc = torch.full((65, B), -1.0, dtype=torch.float64, device="cuda")
    feas = torch.full((65, B), 7, dtype=torch.uint8, device="cuda")
    best = torch.full((65, 4), -3, dtype=torch.int64, device="cuda")
    bctrl = torch.full((65, n, D), -4.0, dtype=torch.float64, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((arc == -1.0).all() and (feas == 7).all() and (best == -3).all() and (bctrl == -4.0).all())

    def launch(Q, w):
        ch.sample_score_queries(big["knots"], DEG, big["init"][:Q], big["sigma"][:Q], big["limits"][:Q], big["seeds"][:Q], Wc, 0,
                                B, arc, feas, best=best, best_ctrl=bctrl, worlds=w)

    for Q in (0, 65):
        with pytest.raises(S.SsppError, match=E_INVAL + ".*sspp_chain_sample_score_worlds"):
            launch(Q, worlds[:Q].reshape(Q, c["nq"]))
        assert untouched()
    for bad_value, what in ((np.nan, "non-finite"), (0.0, "zero quaternion")):
        bad = worlds[:5].copy()
        bad[2, c["block"] + 3:c["block"] + 7] = bad_value
        with pytest.raises(S.SsppError, match=E_INVAL + ".*world 2.*" + what):
            launch(5, bad)
        assert untouched()
    with pytest.raises(ValueError):
        launch(5, worlds[:5, :-1])
    with pytest.raises(S.SsppError, match=E_INVAL + ".*nq = 14"):
        ch.set_qpos(c["qpos0"][:-1])
    zero = c["qpos0"].copy()
    zero[c["block"] + 3:] = 0.0
    with pytest.raises(S.SsppError, match=E_INVAL + ".*zero quaternion"):
        ch.set_qpos(zero)
    with pytest.raises(S.SsppError, match=E_INVAL + ".*out of range"):
        ch.set_body_pose(len(c["names"]), (0, 0, 0), (1, 0, 0, 0))
    assert ch.epoch == 0 and untouched()
    np.testing.assert_array_equal(ch.get_qpos(), c["qpos0"])
    with pytest.raises(S.SsppError, match=E_INVAL + ".*world 2"):
        bad = worlds[:5].copy()
        bad[2, 6] = np.inf
        ch.plan_many(np.zeros((5, D)), np.ones((5, D)) * 0.1, 0.1, np.full(D, np.pi), 16, 20, 5, worlds=bad)
    launch(64, worlds[:64])  # (the largest set is served)
    assert not untouched()
