"""The contact report on the GPU (sspp_scene_contacts, sspp_job_path_contacts and the surfaces over
them) against tests/contact_report_ref.py, against the stand-alone host program byte for byte, and
against the scoring kernels' own decisions (exact agreement: a mismatch is a finding about one of
the two kernels).  Poses, seeds and references are tests/test_contact_report_host.py's.
"""
import os

import numpy as np
import pytest

from oracle import mjcf_ref
from oracle import oracle as O
from tests import capsule_scenes as CS
from tests import contact_report_ref as CRR
from tests import scene_update_worlds as Wd
from tests import synth_scenes as Y
from tests import test_contact_report_host as H

pytestmark = pytest.mark.gpu

GUARD = 64
N_PREFIXES = (1, 63, 64, 65, 257)
GRIPPER_OFFSET = np.array([0.5, 0.05, 0.0, 0.0])  # the BODY recipe centred on robocrane's brick stack


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def S(cuda):
    import sspp_amd
    return sspp_amd


@pytest.fixture(scope="module")
def exe(cuda, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("contact_report_gpu") / "check_report")
    r = H._build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def host_cases(tmp_path_factory):
    """test_contact_report_host's scenes: model, poses, reference — computed once"""
    tmp = tmp_path_factory.mktemp("contact_report_gpu_scenes")
    made = {}

    def get(name):
        if name not in made:
            _, scene, mode, arg, seed, want = next(s for s in H.SCENES if s[0] == name)
            text = scene()
            ref = H.load(tmp, name + "_ref", text)
            xml = os.path.join(str(tmp), name + ".xml")
            with open(xml, "w") as f:
                f.write(text if isinstance(text, str) else CS.mjcf(*text))
            if isinstance(arg, str):
                arg = ref["body_names"].index(arg)
            qs = H.poses_for(ref, mode, arg, seed)
            pairs = CRR.columns(ref, mode, arg)
            contact, deep, near = CRR.pair_counts(ref, mode, arg, pairs, qs)
            for a in (qs, contact, deep, near):
                a.setflags(write=False)
            made[name] = dict(ref=ref, xml=xml, mode=mode, arg=arg, qs=qs, pairs=pairs, contact=contact, deep=deep,
                              near=near, want=want, tmp=tmp)
        return made[name]

    return get


def guarded(torch, shape):
    """a uint8 device tensor of `shape` inside a buffer with GUARD bytes of 0xA5 on both sides"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_ok(buf):
    b = _np(buf)
    return (b[:GUARD] == 0xA5).all() and (b[-GUARD:] == 0xA5).all()


def raw_contacts(S, scene, q, deep=True):
    """sspp_scene_contacts into guarded buffers: (contact, deep) as numpy, guards asserted"""
    import ctypes as C
    import torch
    from sspp_amd import _lib
    N, P = int(q.shape[0]), scene.info()["n_pairs"]
    dq = torch.from_numpy(np.array(q, np.float64)).cuda()
    cb, c = guarded(torch, (N, P))
    db, d = guarded(torch, (N, P))
    c.fill_(0x5A)
    d.fill_(0x5A)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    rc = _lib.lib().sspp_scene_contacts(scene.handle, C.c_void_p(dq.data_ptr()) if N else None, N,
                                        vp(c) if N * P else None, vp(d) if deep and N * P else None,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert guards_ok(cb) and guards_ok(db)
    return _np(c), _np(d)


# ------------------------------------------------------------------ 1. pose form against the reference
@pytest.mark.parametrize("name", ["zoo", "zoo_d3", "zoo_d6", "two_movers", "grid", "tsp_boxes", "tsp_cylinders", "capsule",
                                  "cylcyl"])
def test_pose_form_against_reference(S, host_cases, name):
    c = host_cases(name)
    CRR.assert_not_vacuous(c["ref"], c["pairs"], c["contact"], c["deep"], H.MIN_EACH.get(name, 4), want_multi=c["want"][0],
                           want_deep_gt=c["want"][1], want_shallow=c["want"][2])
    assert c["near"].sum() <= CRR.MAX_NEAR
    scene = S.Scene(S.Model(c["xml"]), c["mode"], c["arg"])
    got = scene.pairs()
    assert [(p["geom1"], p["geom2"]) for p in got] == c["pairs"]
    names = c["ref"]["geom_names"]
    assert all(p["name1"] == names[p["geom1"]] and p["name2"] == names[p["geom2"]] for p in got)
    assert all(p["type1"] == c["ref"]["geom_type"][p["geom1"]] for p in got)
    P = len(c["pairs"])
    assert P == {"zoo": 11, "zoo_d3": 11, "zoo_d6": 11, "two_movers": 12, "grid": 72}.get(name, P)
    ct, dp = raw_contacts(S, scene, c["qs"])
    for n in N_PREFIXES:
        a, b = raw_contacts(S, scene, c["qs"][:n])
        keep = ~c["near"][:n]
        np.testing.assert_array_equal(a[keep], c["contact"][:n][keep])
        np.testing.assert_array_equal(b[keep], c["deep"][:n][keep])
        assert np.array_equal(a, ct[:n]) and np.array_equal(b, dp[:n])   # prefixes of one answer
        only_c, untouched = raw_contacts(S, scene, c["qs"][:n], deep=False)     # d_deep = NULL
        assert np.array_equal(only_c, a) and (untouched == 0x5A).all()
    # the Python surface
    tc, td = scene.contacts(c["qs"])
    assert np.array_equal(_np(tc), ct) and np.array_equal(_np(td), dp)
    tc2, none = scene.contacts(c["qs"], deep=False)
    assert none is None and np.array_equal(_np(tc2), ct)


def gripper_case(S):
    """robocrane's gripper as a TaskSpacePlanner body: 48 pairs; the per-pair reference on the
    scene's own column list (nested bodies and excludes: the product's filter is checked through
    the column sums against the whole-scene oracle)."""
    ref = mjcf_ref.load(Wd.ROBOCRANE)
    body = ref["body_names"].index(Wd.GRIPPER)
    scene = S.Scene(S.Model(Wd.ROBOCRANE), 1, body)
    pairs = [(p["geom1"], p["geom2"]) for p in scene.pairs()]
    qs = CRR.body_poses(1) + GRIPPER_OFFSET
    return ref, body, scene, pairs, qs


def test_pose_form_robocrane_gripper(S):
    ref, body, scene, pairs, qs = gripper_case(S)
    assert len(pairs) == 48
    contact, deep, near = CRR.pair_counts(ref, 1, body, pairs, qs)
    assert not near.any()
    assert ((contact > 0).any(1)).sum() >= 4 and ((contact == 0).all(1)).sum() >= 4 and (deep > contact).any()
    whole = O.Scene(ref, 1, body)
    tot = np.array([whole.contacts(q)[::2] for q in qs])
    np.testing.assert_array_equal(contact.sum(1), tot[:, 0])
    np.testing.assert_array_equal(deep.sum(1), tot[:, 1])
    for n in N_PREFIXES:
        ct, dp = raw_contacts(S, scene, qs[:n])
        np.testing.assert_array_equal(ct, contact[:n])
        np.testing.assert_array_equal(dp, deep[:n])


def test_scene_without_pairs_writes_nothing(S, tmp_path):
    """a mover whose only geom shares no bit with anything: P = 0, SSPP_OK, nothing written"""
    xml = tmp_path / "lonely.xml"
    xml.write_text(Y.mjcf([Y.ramp()], [Y.body("mover", (0, 0, 0.3), [Y.geom(Y.BOX, Y.MOVER_BOX, name="m", contype=2,
                                                                                 conaffinity=2)])]))
    scene = S.Scene(S.Model(str(xml)), 0, 7)
    assert scene.info()["n_pairs"] == 0 and scene.pairs() == []
    ct, dp = raw_contacts(S, scene, CRR.qpos_poses(1, 65))
    assert ct.shape == (65, 0) and dp.shape == (65, 0)
    c, d = scene.contacts(CRR.qpos_poses(1, 5))
    assert tuple(c.shape) == (5, 0)


# ------------------------------------------------------------------ 2. bit-equal to the host routine
@pytest.mark.parametrize("name", ["zoo", "zoo_d3", "zoo_d6", "two_movers", "grid", "tsp_boxes", "tsp_cylinders", "capsule",
                                  "cylcyl"])
def test_pose_form_equals_host_routine(S, exe, host_cases, name):
    c = host_cases(name)
    inp = os.path.join(str(c["tmp"]), name + ".in")
    H.write_input(inp, c["ref"], c["mode"], c["arg"], c["qs"])
    h = H.run(exe, inp)
    scene = S.Scene(S.Model(c["xml"]), c["mode"], c["arg"])
    ct, dp = raw_contacts(S, scene, c["qs"])
    assert ct.tobytes() == h["contact"].tobytes() and dp.tobytes() == h["deep"].tobytes()
    sp = scene.static_pairs()
    assert [(p["geom1"], p["geom2"], p["contact"], p["deep"]) for p in sp] == [(a, b, x, y) for a, b, _, x, y in h["spairs"]]


# ------------------------------------------------------------------ 3. path form, SamplingPathPlanner
def linear_init(start, end, n):
    u = np.array([i / (n - 1) for i in range(n)])
    return O.interpolate(np.array([(1 - t) * start + t * end for t in u]), 3, u)


@pytest.mark.parametrize("D", [7, 3, 6])   # 3, 6: undriven entries of the mover from the scene's defaults
@pytest.mark.parametrize("W", [1, 16])
def test_sspp_path_form(S, host_cases, W, D):
    import torch
    from sspp_amd import _lib
    c = host_cases("zoo")
    B, n = 33, 10
    lift = np.array([0, 0, 0.08, 0, 0, 0, 0])   # over the statics' tops: some candidates pass, some do not
    limits = Y.ZOO_LIMITS[:D]
    knots, ctrl0 = linear_init((Y.ZOO_START + lift)[:D], (Y.ZOO_END + lift)[:D], n)
    ctrl = O.sample_sspp(ctrl0, 3, 0.12, limits, 7, 0, B)
    scene = S.Scene(S.Model(c["xml"]), 0, D)
    P = scene.info()["n_pairs"]
    job = S.SsppJob(scene, knots, 3, ctrl0, 0.12, limits, W, max_batch=B)
    dctrl = torch.from_numpy(ctrl).cuda()
    pc, pd = job.path_contacts(dctrl)
    assert tuple(pc.shape) == (B, W + 1, P) and tuple(pd.shape) == (B, W + 1, P)
    pc, pd = _np(pc), _np(pd)
    # the pose form on the oracle's waypoints
    wp = np.array([[O.spline_eval(knots, 3, ctrl[b], i / W) for i in range(W + 1)] for b in range(B)])
    qc, qd = scene.contacts(wp.reshape(-1, D))
    assert np.array_equal(pc.reshape(-1, P), _np(qc)) and np.array_equal(pd.reshape(-1, P), _np(qd))
    hit = pc.reshape(B, -1).any(1)
    if W == 16:   # (the oracle scores W >= 2 only)
        feas_o = O.sspp_score(O.Scene(c["ref"], 0, D), knots, 3, ctrl, W)[1].astype(bool)
        assert 4 <= feas_o.sum() <= B - 4, feas_o.sum()      # from the reference alone
        np.testing.assert_array_equal(~hit, feas_o)
    static_free = scene.info()["static_contacts"] == 0
    for f32 in (1, 0):
        for order in (0, 1, 2):
            job.set_option(_lib.OPT_F32, f32)
            job.set_option(_lib.OPT_ORDER, order)
            o = job.alloc(B)
            job.score_ctrl(dctrl, 0, o["arc"], o["feasible"], o["best"])
            torch.cuda.synchronize()
            feas = _np(o["feasible"]).astype(bool)
            np.testing.assert_array_equal(feas, static_free & ~hit, err_msg="f32 %d order %d" % (f32, order))
            again, _ = job.path_contacts(dctrl, deep=False)   # columns do not follow the job's scan order
            assert np.array_equal(_np(again), pc)


# ------------------------------------------------------------------ 4. path form, TaskSpacePlanner
def tsp_case(S, host_cases, which):
    if which == "tsp_boxes":
        c = host_cases("tsp_boxes")
        ref, body, scene = c["ref"], c["arg"], S.Scene(S.Model(c["xml"]), 1, c["arg"])
        return ref, body, scene, Y.TSP_START, Y.TSP_END, Y.TSP_LO, Y.TSP_HI
    if which == "stacking":   # every box upright: the scoring kernels' upright forms (sspr::kUpright)
        ref = mjcf_ref.load(Wd.STACKING)
        body = ref["body_names"].index("block1")
        return (ref, body, S.Scene(S.Model(Wd.STACKING), 1, body), np.array([0.205, 0.0, 0.12, 0.0]),
                np.array([0.0, 0.0, 0.32, 0.0]), Y.TSP_LO, Y.TSP_HI)
    ref, body, scene, _, _ = gripper_case(S)
    off = GRIPPER_OFFSET
    return ref, body, scene, Y.TSP_START + off, Y.TSP_END + off, Y.TSP_LO + off, Y.TSP_HI + off


@pytest.mark.parametrize("which", ["tsp_boxes", "gripper", "stacking"])
@pytest.mark.parametrize("cp", [17, 40])
def test_tsp_path_form(S, host_cases, which, cp):
    import torch
    from sspp_amd import _lib
    ref, body, scene, start, end, lo, hi = tsp_case(S, host_cases, which)
    B, K = 33, 2
    P = scene.info()["n_pairs"]
    mean = np.stack([start + (end - start) * (k + 1) / (K + 1) for k in range(K)])
    # (sigma, seed): chosen so that the oracle alone shows converged and colliding via sets
    sg, seed = (0.3, 12) if which == "stacking" else (0.15, 11)
    sigma = np.full((K, 4), sg)
    vias = O.sample_tsp(mean, sigma, lo, hi, 0.0, seed, 0, B)
    whole = O.Scene(ref, 1, body)
    st_o = O.tsp_score(whole, start, end, vias, cp)[3]
    assert 4 <= st_o.sum() <= B - 4, st_o.sum()
    job = S.TspJob(scene, start, end, K, cp, mean=mean, sigma=sigma, lo=lo, hi=hi, seed=seed, max_batch=B)
    dv = torch.from_numpy(vias).cuda()
    pc, pd = job.path_contacts(dv)
    assert tuple(pc.shape) == (B, cp, P)
    pc, pd = _np(pc), _np(pd)
    clean = ~pd.reshape(B, -1).any(1)
    np.testing.assert_array_equal(clean, st_o == 1)
    static_free = scene.info()["static_cost"] == 0.0
    assert static_free
    for form in (-1, 0):
        job.set_option(_lib.OPT_TSP_FORM, form)
        o = job.alloc(B)
        job.score_vias(dv, 0, o["L"], o["Cnf"], o["Cwf"], o["status"], o["cost"], o["best"])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(o["status"]) == 1, static_free & clean, err_msg="form %d" % form)
        np.testing.assert_array_equal(_np(o["Cnf"]) == 0.0, static_free & clean)
    # column sums over pairs: the oracle's nd per waypoint (waypoints: the oracle's interpolation)
    pts = np.concatenate([np.broadcast_to(start, (B, 1, 4)), vias, np.broadcast_to(end, (B, 1, 4))], 1)
    u = np.array([i / (K + 1) for i in range(K + 2)])
    for b in range(B):
        knots, ctrl = O.interpolate(pts[b], 2, u)
        nd = [whole.contacts(O.spline_eval(knots, 2, ctrl, i / cp))[2] for i in range(1, cp + 1)]
        np.testing.assert_array_equal(pd[b].sum(1), nd)


# ------------------------------------------------------------------ 5. scene updates
def snapshot(S, scene, qs):
    out = dict(pairs=scene.pairs(), static=scene.static_pairs())
    c, d = scene.contacts(qs)
    out["contact"], out["deep"] = _np(c).tobytes(), _np(d).tobytes()
    return out


def test_reposed_scene_reports_as_a_fresh_one(S, tmp_path):
    import torch
    md0 = mjcf_ref.load(Wd.ROBOCRANE)
    scene = S.Scene(S.Model(Wd.ROBOCRANE), 0, 7)
    rng = np.random.default_rng(3)
    qs = np.concatenate([np.stack([rng.uniform(0.3, 0.7, 65), rng.uniform(-0.15, 0.25, 65), rng.uniform(0.1, 0.5, 65)], 1),
                         np.tile([0.707, 0, 0, 0.707], (65, 1))], 1)
    knots, ctrl0 = linear_init(Wd.START7, Wd.END7, 10)
    ctrl = torch.from_numpy(O.sample_sspp(ctrl0, 3, 0.08, np.ones(7), 5, 0, 9)).cuda()
    job = S.SsppJob(scene, knots, 3, ctrl0, 0.08, np.ones(7), 16, max_batch=9)
    seen = []
    for w in ("W1", "N", "W2"):
        edits = Wd.CRANE[w]
        for name, (pos, quat) in edits.items():
            b = md0["body_names"].index(name)
            scene.set_body_pose(name, pos, quat if quat is not None else md0["body_quat"][b])
        world = dict(e for ww in seen + [w] for e in Wd.CRANE[ww].items())
        fresh = S.Scene(S.Model(Wd.write_xml(Wd.ROBOCRANE, tmp_path / (w + ".xml"), world)), 0, 7)
        a, f = snapshot(S, scene, qs), snapshot(S, fresh, qs)
        assert a == f, w
        fjob = S.SsppJob(fresh, knots, 3, ctrl0, 0.08, np.ones(7), 16, max_batch=9)
        (c1, d1), (c2, d2) = job.path_contacts(ctrl), fjob.path_contacts(ctrl)
        assert _np(c1).tobytes() == _np(c2).tobytes() and _np(d1).tobytes() == _np(d2).tobytes()
        seen.append(w)


def test_set_qpos_reports_as_a_fresh_scene(S, tmp_path):
    """the same through set_qpos (the whole qpos: the gripper next to the stack, the gripper in the
    floor, a free brick pushed into the wall), on sspp_amd.Scene and on the drop-in planner"""
    import torch
    from sspp import _sspp
    md0 = mjcf_ref.load(Wd.ROBOCRANE)
    scene = S.Scene(S.Model(Wd.ROBOCRANE), 0, 7)
    sp = _sspp.SamplingPathPlanner7(Wd.ROBOCRANE)
    rng = np.random.default_rng(3)
    qs = np.concatenate([np.stack([rng.uniform(0.3, 0.7, 65), rng.uniform(-0.15, 0.25, 65), rng.uniform(0.1, 0.5, 65)], 1),
                         np.tile([0.707, 0, 0, 0.707], (65, 1))], 1)
    knots, ctrl0 = linear_init(Wd.START7, Wd.END7, 10)
    ctrl = torch.from_numpy(O.sample_sspp(ctrl0, 3, 0.08, np.ones(7), 5, 0, 9)).cuda()
    job = S.SsppJob(scene, knots, 3, ctrl0, 0.08, np.ones(7), 16, max_batch=9)
    path = _sspp.Spline7()
    sp.initializePath(Wd.START7, Wd.END7, path, 10)
    worlds = [("N", Wd.CRANE["N"]), ("F", Wd.CRANE["F"]), ("brick", {ORANGE_ON_WALL[0]: ORANGE_ON_WALL[1:]}), ("A", {})]
    statics = {}
    for w, edits in worlds:
        q = Wd.qpos_for(md0, edits)
        scene.set_qpos(q)
        xml = Wd.write_xml(Wd.ROBOCRANE, tmp_path / (w + ".xml"), edits)
        fresh = S.Scene(S.Model(xml), 0, 7)
        a, f = snapshot(S, scene, qs), snapshot(S, fresh, qs)
        assert a == f, w
        fjob = S.SsppJob(fresh, knots, 3, ctrl0, 0.08, np.ones(7), 16, max_batch=9)
        (c1, d1), (c2, d2) = job.path_contacts(ctrl), fjob.path_contacts(ctrl)
        assert _np(c1).tobytes() == _np(c2).tobytes() and _np(d1).tobytes() == _np(d2).tobytes()
        statics[w] = sum(p["contact"] for p in a["static"])
        assert statics[w] == scene.info()["static_contacts"]
        sp.set_qpos(q)
        rows = lambda r: [(i, None if i < 0 else u, g1, g2, n) for i, u, g1, g2, n in r]  # noqa: E731 (u = nan for statics)
        got, want = rows(sp.contact_report(path, 16)), rows(_sspp.SamplingPathPlanner7(xml).contact_report(path, 16))
        assert got == want and bool(got) == sp.checkCollision(path, 16, None), w
    assert statics == {"N": 0, "F": 8, "brick": 1, "A": 0}     # (F: the oracle's 8, tests/test_scene_update_host.py)


def test_reposed_body_scene_reports_as_a_fresh_one(S, tmp_path):
    """a TaskSpacePlanner scene (stacking.xml, block1 moving): pairs, static pairs, the pose form and
    TspJob.path_contacts after set_body_pose / set_qpos equal a fresh scene's and a fresh job's"""
    import torch
    md0 = mjcf_ref.load(Wd.STACKING)
    scene = S.Scene(S.Model(Wd.STACKING), 1, "block1")
    start, end = np.array([0.205, 0.0, 0.12, 0.0]), np.array([0.0, 0.0, 0.32, 0.0])
    K, cp, B = 2, 17, 9
    mean = np.stack([start + (end - start) * (k + 1) / (K + 1) for k in range(K)])
    sigma = np.full((K, 4), 0.3)
    vias = torch.from_numpy(O.sample_tsp(mean, sigma, Y.TSP_LO, Y.TSP_HI, 0.0, 12, 0, B)).cuda()
    kw = dict(mean=mean, sigma=sigma, lo=Y.TSP_LO, hi=Y.TSP_HI, seed=12, max_batch=B)
    job = S.TspJob(scene, start, end, K, cp, **kw)
    qs = CRR.body_poses(1, 65)
    seen = {}
    for w, by_qpos in (("S1", False), ("S2", True), ("S1", True), ("S2", False), ("A", True)):
        edits = Wd.STACK[w]
        if by_qpos:
            scene.set_qpos(Wd.qpos_for(md0, edits))
        else:
            for name, (pos, quat) in dict({"block3": Wd.BLOCK3_A}, **edits).items():
                scene.set_body_pose(name, pos, quat)
        fresh = S.Scene(S.Model(Wd.write_xml(Wd.STACKING, tmp_path / (w + ".xml"), edits)), 1, "block1")
        a, f = snapshot(S, scene, qs), snapshot(S, fresh, qs)
        assert a == f, (w, by_qpos)
        fjob = S.TspJob(fresh, start, end, K, cp, **kw)
        (c1, d1), (c2, d2) = job.path_contacts(vias), fjob.path_contacts(vias)
        assert _np(c1).tobytes() == _np(c2).tobytes() and _np(d1).tobytes() == _np(d2).tobytes(), (w, by_qpos)
        key = (a["contact"], a["deep"], str(a["static"]))
        assert seen.setdefault(w, key) == key
    assert len({seen[w] for w in seen}) == 3      # not vacuous: the three worlds report differently


ORANGE_ON_WALL = ("block_orange/", (0.5, 0.05, 0.19), Wd.IDENT)   # a free brick, static for dof 7, into the wall's top brick


def test_stacked_static_bricks_are_named(S, cuda):
    """A re-planning loop that moves a brick into another: the env-env pair shows in static_pairs()
    and leads the drop-ins' reports.  robocrane.xml for SamplingPathPlanner7 (block_orange into the
    wall's block_magenta), stacking.xml's S2 for the TaskSpacePlanner (block3 into block2)."""
    from sspp import _sspp, _tsp
    pair = {"block_orange/block_orange_geom", "lego_bricks_1/block_magenta_geom"}
    scene = S.Scene(S.Model(Wd.ROBOCRANE), 0, 7)
    assert scene.info()["static_contacts"] == 0 and not [p for p in scene.static_pairs() if p["contact"]]
    scene.set_body_pose(*ORANGE_ON_WALL)
    touching = [p for p in scene.static_pairs() if p["contact"]]
    assert [({p["name1"], p["name2"]}, p["contact"]) for p in touching] == [(pair, 1)] and touching[0]["deep"] == 4
    assert sum(p["contact"] for p in scene.static_pairs()) == scene.info()["static_contacts"] == 1
    sp = _sspp.SamplingPathPlanner7(Wd.ROBOCRANE)
    path = _sspp.Spline7()
    sp.initializePath(Wd.START7 + np.array([0, 0, 0.3, 0, 0, 0, 0]), Wd.END7 + np.array([0, 0, 0.3, 0, 0, 0, 0]), path, 10)
    assert sp.contact_report(path, 8) == [] and not sp.checkCollision(path, 8, None)
    sp.set_body_pose(*ORANGE_ON_WALL)
    rep = sp.contact_report(path, 8)
    assert rep and rep[0][0] == -1 and np.isnan(rep[0][1]) and set(rep[0][2:4]) == pair and rep[0][4] == 1
    assert sp.checkCollision(path, 8, None)

    md0 = mjcf_ref.load(Wd.STACKING)
    bricks = {"block2_geom", "block3_geom"}
    tscene = S.Scene(S.Model(Wd.STACKING), 1, "block1")
    assert not [p for p in tscene.static_pairs() if {p["name1"], p["name2"]} == bricks and p["contact"]]
    (pos, quat), = Wd.STACK["S2"].values()
    tscene.set_body_pose("block3", pos, quat)
    hit, = [p for p in tscene.static_pairs() if {p["name1"], p["name2"]} == bricks]
    assert hit["contact"] >= 1 and hit["deep"] >= 1
    assert sum(p["contact"] for p in tscene.static_pairs()) == tscene.info()["static_contacts"]
    pl = _tsp.TaskSpacePlanner(Wd.STACKING, "block1", sample_count=64, check_points=16)
    far = np.array([0.45, 0.45, 0.58, 0.0])
    assert not pl.check_collision_point(far) and pl.contact_report(far) == []
    pl.set_body_pose("block3", pos, quat)
    rep = pl.contact_report(far)
    assert rep and set(rep[0][:2]) == bricks and rep[0][2] == hit["deep"] and pl.check_collision_point(far)
    assert md0["geom_names"].index(rep[0][0]) < md0["geom_names"].index(rep[0][1])


# ------------------------------------------------------------------ 6. drop-ins
def test_dropin_contact_report_equals_check_collision(S, cuda):
    from sspp import _sspp
    md = mjcf_ref.load(Wd.ROBOCRANE)
    sp = _sspp.SamplingPathPlanner7(Wd.ROBOCRANE)
    hits = 0
    names = set(md["geom_names"])
    init = _sspp.Spline7()
    sp.initializePath(Wd.START7, Wd.END7, init, 10)
    for i in range(32):
        s = sp.sampleWithNoise(init, 0.08, np.ones(7), i)
        rep = sp.contact_report(s, 16)
        assert bool(rep) == sp.checkCollision(s, 16, None)
        hits += bool(rep)
        for wpt, u, n1, n2, cnt in rep:
            assert n1 in names and n2 in names and md["geom_names"].index(n1) < md["geom_names"].index(n2)
            assert 0 <= wpt <= 16 and u == wpt / 16 and cnt >= 1
        assert rep == sorted(rep, key=lambda r: r[0])
    assert 2 <= hits <= 30, hits


def test_dropin_check_collision_point(S, cuda):
    from sspp import _tsp
    ref = mjcf_ref.load(Wd.STACKING)
    body = ref["body_names"].index("block1")
    whole = O.Scene(ref, 1, body)
    pl = _tsp.TaskSpacePlanner(Wd.STACKING, "block1", sample_count=64, check_points=16)
    qs = CRR.body_poses(1, 64)
    want = [whole.contacts(q, count_static=True)[2] > 0 for q in qs]
    got = [pl.check_collision_point(q) for q in qs]
    assert got == want and 4 <= sum(want) <= 60, sum(want)
    for q, w in zip(qs[:16], want[:16]):
        rep = pl.contact_report(q)
        assert bool(rep) == w and sum(r[2] for r in rep) == whole.contacts(q, count_static=True)[2]


# ------------------------------------------------------------------ 7. errors
def test_errors_leave_the_objects_usable(S, host_cases):
    import ctypes as C
    import torch
    from sspp_amd import _lib
    L = _lib.lib()
    c = host_cases("zoo")
    scene = S.Scene(S.Model(c["xml"]), 0, 7)
    P = scene.info()["n_pairs"]
    q = torch.from_numpy(np.array(c["qs"][:8])).cuda()
    out = torch.zeros((8, P), dtype=torch.uint8, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.sspp_scene_contacts(scene.handle, None, 8, vp(out), None, None) == -1 and "null" in _lib.last_error()
    assert L.sspp_scene_contacts(scene.handle, vp(q), 8, None, None, None) == -1 and "null" in _lib.last_error()
    assert L.sspp_scene_contacts(None, vp(q), 8, vp(out), None, None) == -1 and _lib.last_error()
    assert L.sspp_scene_contacts(scene.handle, None, 0, None, None, None) == 0            # N = 0: nothing to do
    n = C.c_int()
    infos = (_lib.PairInfo * P)()
    assert L.sspp_scene_pairs(scene.handle, infos, P - 1, C.byref(n)) == -1 and "cap" in _lib.last_error() and n.value == P
    assert L.sspp_scene_pairs(scene.handle, None, 0, C.byref(n)) == 0 and n.value == P
    assert L.sspp_scene_pairs(scene.handle, infos, P, C.byref(n)) == 0
    rscene = S.Scene(S.Model(Wd.ROBOCRANE), 0, 7)      # (the zoo's statics share the world body: no env-env pair)
    ns = rscene.info()["n_static_pairs"]
    assert ns > 0
    sinfos, sc8, sd8 = (_lib.PairInfo * ns)(), (C.c_uint8 * ns)(), (C.c_uint8 * ns)()
    assert L.sspp_scene_static_pairs(rscene.handle, sinfos, sc8, sd8, ns - 1, C.byref(n)) == -1
    assert "cap" in _lib.last_error() and n.value == ns
    assert L.sspp_scene_static_pairs(rscene.handle, None, sc8, None, 0, C.byref(n)) == -1      # counts alone need room too
    assert L.sspp_scene_static_pairs(rscene.handle, sinfos, sc8, sd8, ns, C.byref(n)) == 0
    with pytest.raises(S.SsppError, match=r"\(-1\)"):
        scene.contacts(np.zeros((4, 6)))
    a, b = scene.contacts(c["qs"][:8])
    assert np.array_equal(_np(a), c["contact"][:8]) and np.array_equal(_np(b), c["deep"][:8])

    knots, ctrl0 = linear_init(Y.ZOO_START, Y.ZOO_END, 10)
    job = S.SsppJob(scene, knots, 3, ctrl0, 0.1, Y.ZOO_LIMITS, 8, max_batch=4)
    ctrl = torch.from_numpy(np.tile(ctrl0, (4, 1, 1))).cuda()
    pout = torch.zeros((4, 9, P), dtype=torch.uint8, device="cuda")
    assert L.sspp_job_path_contacts(job._h, None, 4, vp(pout), None, None) == -1 and "null" in _lib.last_error()
    assert L.sspp_job_path_contacts(None, vp(ctrl), 4, vp(pout), None, None) == -1 and _lib.last_error()
    with pytest.raises(S.SsppError, match=r"\(-1\)"):
        job.path_contacts(ctrl[:, :9])
    good = _np(job.path_contacts(ctrl)[0])
    assert good.shape == (4, 9, P)

    c2 = host_cases("tsp_boxes")
    tscene = S.Scene(S.Model(c2["xml"]), 1, c2["arg"])
    tjob = S.TspJob(tscene, Y.TSP_START, Y.TSP_END, 2, 17, lo=Y.TSP_LO, hi=Y.TSP_HI, max_batch=4)
    with pytest.raises(S.SsppError, match=r"\(-1\)"):
        tjob.path_contacts(np.zeros((4, 3, 4)))                    # K = 2: the wrong path shape
    with pytest.raises(S.SsppError, match=r"\(-1\)"):
        tjob.path_contacts(np.zeros((4, 2, 7)))
    vias = np.tile(np.stack([Y.TSP_START, Y.TSP_END]) * 0.5, (4, 1, 1))
    assert tuple(tjob.path_contacts(vias)[0].shape) == (4, 17, tscene.info()["n_pairs"])

    # a job whose scene was freed first
    doomed = S.Scene(S.Model(c["xml"]), 0, 7)
    djob = S.SsppJob(doomed, knots, 3, ctrl0, 0.1, Y.ZOO_LIMITS, 8, max_batch=4)
    L.sspp_scene_free(doomed.handle)
    doomed._h = None
    assert L.sspp_job_path_contacts(djob._h, vp(ctrl), 4, vp(pout), None, None) == -3 and "scene" in _lib.last_error()
    assert np.array_equal(_np(job.path_contacts(ctrl)[0]), good)    # a following valid call works
