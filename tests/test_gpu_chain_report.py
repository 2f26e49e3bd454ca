"""The contact report for arms on the GPU (sspp_chain_pair_contacts / _path_contacts /
_first_contacts / _static_pairs and the Chain methods) against the stand-alone host program byte for
byte (tests/chain_report/check_chain_report.cpp runs the same __host__ __device__ routines), against
each other (a path row is the pose report of its waypoint, a first contact is the dense report's
first nonzero entry) and against the chain's own decisions (Chain.contacts, Chain.score_ctrl).  The
host program itself is checked against numpy in tests/test_chain_report_host.py.
"""
import ctypes as C

import numpy as np
import pytest

from tests import chain_host as H
from tests import chain_report_host as RH
from tests import chain_scenes as W
from tests import test_chain_report_host as TRH
from tests import test_gpu_chain as TG
from tests.test_gpu_scene_update import live_resources

pytestmark = pytest.mark.gpu

_np = TG._np


@pytest.fixture(scope="module")
def S(cuda):
    import sspp_amd
    return sspp_amd


@pytest.fixture(scope="module")
def exe(cuda, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chain_report_gpu") / "check_chain_report")
    r = RH.build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def exe_chain(cuda, tmp_path_factory):
    """tests/chain/check_chain.cpp, for tests/test_gpu_chain.py's helpers (free_poses, random_splines)"""
    out = str(tmp_path_factory.mktemp("chain_report_gpu_old") / "check_chain")
    r = H.build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("chain_report_gpu_worlds")


@pytest.fixture(scope="module")
def arms(S, tmp):
    made = {}

    def get(name):
        if name not in made:
            nj, seed, fb = TG.ARMS[name]
            world = TG.arm_world(nj, seed, fb)
            xml = H.write_xml(tmp, name, W.mjcf(world))
            made[name] = dict(world=world, xml=xml, model=S.Model(xml, joints=True), fb=fb, seed=seed)
        return made[name]

    return get


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


# ------------------------------------------------------------------ 1. pair_contacts
@pytest.mark.parametrize("name,D", TG.FK_CASES)
def test_pair_contacts_equal_host_bytes(S, exe, tmp, arms, name, D):
    a = arms(name)
    q = W.arm_poses(D, max(TG.N_SIZES), a["seed"] + 7, 2.0, a["fb"])
    host = RH.chain(exe, a["xml"], D, q, tmp, tag="%s_%d" % (name, D))
    assert host["rc"] == 0, host["err"]
    ch = S.Chain(a["model"], D, count_static=False)
    P = ch.info()["n_pairs"]
    assert [(p["geom1"], p["geom2"], int(p["moving1"]), int(p["moving2"]), p["margin"]) for p in ch.pairs()] == host["pairs"]
    assert [(p["geom1"], p["geom2"], p["margin"], p["contact"], p["deep"]) for p in ch.static_pairs()] == host["statics"]
    assert (host["contact"] > 0).any() and (host["contact"] == 0).all(1).any()  # (both decisions occur)
    dq = dev(q)
    for N in TG.N_SIZES:
        c, d = ch.pair_contacts(dq[:N])
        assert c.shape == d.shape == (N, P)
        assert _np(c).tobytes() == host["contact"][:N].tobytes(), (name, D, N)
        assert _np(d).tobytes() == host["deep"][:N].tobytes(), (name, D, N)
        c1, d1 = ch.pair_contacts(dq[:N], deep=False)
        assert d1 is None and _np(c1).tobytes() == host["contact"][:N].tobytes(), (name, D, N)
        assert np.array_equal((_np(c) > 0).any(1), _np(ch.contacts(dq[:N])).astype(bool))
    c, d = ch.pair_contacts(dq[:0])
    assert c.shape == d.shape == (0, P)


@pytest.mark.parametrize("offset", [1, 7, 15])
def test_pair_contacts_into_unaligned_outputs(S, exe, tmp, arms, offset):
    """outputs that do not start on a 16-byte boundary (the copy's single bytes before the first and
    after the last boundary of each wave's block): the bytes are the host's and nothing beside them
    is written"""
    import torch
    from sspp_amd import _lib
    a = arms("arm7")
    N, D = 130, 7
    q = W.arm_poses(D, N, 5, 2.0)
    host = RH.chain(exe, a["xml"], D, q, tmp, tag="unal")
    ch = S.Chain(a["model"], D, count_static=False)
    P = ch.info()["n_pairs"]
    dq = dev(q)
    for n in (1, 63, 65, N):
        bc = torch.full((n * P + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        bd = torch.full((n * P + 64,), 0xCD, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib().sspp_chain_pair_contacts(ch.handle, C.c_void_p(dq.data_ptr()), n,
                                                       C.c_void_p(bc.data_ptr() + offset),
                                                       C.c_void_p(bd.data_ptr() + 16 - offset),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "pair_contacts")
        torch.cuda.synchronize()
        gc, gd = _np(bc), _np(bd)
        assert gc[offset:offset + n * P].tobytes() == host["contact"][:n].tobytes(), (offset, n)
        assert gd[16 - offset:16 - offset + n * P].tobytes() == host["deep"][:n].tobytes(), (offset, n)
        assert (gc[:offset] == 0xAB).all() and (gc[offset + n * P:] == 0xAB).all()
        assert (gd[:16 - offset] == 0xCD).all() and (gd[16 - offset + n * P:] == 0xCD).all()


def test_count_static_leaves_the_report_unchanged(S, exe, tmp):
    """a world whose statics touch (a static block resting on the floor): Chain.contacts is all ones
    with count_static, the report is the same with and without it, and the static pairs list the contact"""
    xml = H.write_xml(tmp, "static_block", W.mjcf(TRH.static_block_world(0.1)))
    model = S.Model(xml, joints=True)
    q = W.arm_poses(3, 200, 3, 2.0)
    host = RH.chain(exe, xml, 3, q, tmp, tag="static_block")
    on, off = S.Chain(model, 3, count_static=True), S.Chain(model, 3, count_static=False)
    assert on.info()["static_contacts"] == host["info"]["static_contacts"] > 0
    sp = on.static_pairs()
    assert [(p["geom1"], p["geom2"], p["margin"], p["contact"], p["deep"]) for p in sp] == host["statics"]
    assert sum(p["contact"] for p in sp) == on.info()["static_contacts"]
    assert all(not p["moving1"] and not p["moving2"] for p in sp) and {"block"} <= {p["name2"] for p in sp}
    dq = dev(q)
    assert _np(on.contacts(dq)).all() and not _np(off.contacts(dq)).all()
    for ch in (on, off):
        c, d = ch.pair_contacts(dq)
        assert _np(c).tobytes() == host["contact"].tobytes() and _np(d).tobytes() == host["deep"].tobytes()


# ------------------------------------------------------------------ 2., 3. path_contacts, first_contacts
PATH_B = (1, 3, 130)
PATH_CASES = [(arm, degree, n, Wc) for arm in ("arm7", "arm9") for degree in (2, 3) for n in (degree + 1, 10)
              for Wc in (1, 62, 63, 64, 65, 128)]


def waypoints(S, knots, degree, ctrl, Wc):
    """sspp_spline_eval at u = i / W, i = 0..W: [B, W + 1, D]"""
    return np.array([[S.spline_eval(knots, degree, c, i / Wc) for i in range(Wc + 1)] for c in ctrl])


@pytest.mark.parametrize("arm,degree,n,Wc", PATH_CASES)
def test_path_and_first_contacts(S, exe, exe_chain, tmp, arms, arm, degree, n, Wc):
    """B = 1, 3, 130 splines (the first B of one set of 130): the dense path report equals the host
    program's on sspp_spline_eval's waypoints and pair_contacts of those waypoints; first_contacts
    equals the record derived from the dense report, and is -1 exactly where score_ctrl says feasible"""
    a = arms(arm)
    D, Bmax = 7, max(PATH_B)
    ch = S.Chain(a["model"], D, count_static=False)
    P = ch.info()["n_pairs"]
    knots, ctrl = TG.random_splines(S, exe_chain, tmp, a["xml"], D, Bmax, n, degree, 2000 + 7 * Wc + n + degree)
    q = waypoints(S, knots, degree, ctrl, Wc)
    host = RH.chain(exe, a["xml"], D, q.reshape(-1, D), tmp, tag="path")
    assert host["rc"] == 0, host["err"]
    want_c, want_d = host["contact"].reshape(Bmax, Wc + 1, P), host["deep"].reshape(Bmax, Wc + 1, P)
    want_first = RH.path_first(want_c)
    assert (want_first[:, 0] >= 0).any()
    if Wc > 1 and arm == "arm7":  # (both kinds of path occur; the 9-joint arm's paths all touch)
        assert (want_first[:, 0] < 0).any()
    dctrl = dev(ctrl)
    for B in PATH_B:
        c, d = ch.path_contacts(knots, degree, dctrl[:B], Wc)
        assert c.shape == d.shape == (B, Wc + 1, P)
        assert _np(c).tobytes() == want_c[:B].tobytes(), (B, Wc)
        assert _np(d).tobytes() == want_d[:B].tobytes(), (B, Wc)
        c1, d1 = ch.path_contacts(knots, degree, dctrl[:B], Wc, deep=False)
        assert d1 is None and _np(c1).tobytes() == want_c[:B].tobytes()
        first = _np(ch.first_contacts(knots, degree, dctrl[:B], Wc))
        assert first.dtype == np.int32 and first.shape == (B, 2)
        np.testing.assert_array_equal(first, want_first[:B])
        np.testing.assert_array_equal(first, RH.path_first(_np(c)))
        _, feas, _ = TG.run_score(S, ch, knots, degree, ctrl[:B], Wc)
        np.testing.assert_array_equal(first[:, 0] == -1, feas)
    pc, pd = ch.pair_contacts(dev(q.reshape(-1, D)))
    assert _np(pc).tobytes() == want_c.tobytes() and _np(pd).tobytes() == want_d.tobytes()


# first_contacts' passes: 256 of sample_score's candidates at W = 100 (two passes of 64 waypoints).
# The recipe asked for is a linear path from free_poses' free start to its touching end.  A clamped
# spline passes through its last control point and sampleWithNoise leaves the end control points
# alone, so with a touching end every candidate touches at waypoint W at the latest and none could
# be free; and an end pulled back along that line to its last free point leaves the late waypoints
# out of the noise's reach (the sampler's noise is sideways, the obstacle lies ahead).  The end is
# therefore another pose of free_poses' pool: FLOOR_POSE, a free pose whose nominal path is free and
# runs close to the obstacles over its last third, found by scanning the pool with the host program
# alone.  With FLOOR_SIGMA and FLOOR_SEED the host program counts, of 256 candidates, 20 first
# contacts at a waypoint >= 64 (the second pass), 215 below 64 and 21 candidates without any
# (seeds 0xBEEF and 2 give 16 / 221 / 19 and 16 / 213 / 27).
FLOOR_POSE, FLOOR_SIGMA, FLOOR_SEED = 371, 0.04, 1


def test_first_contacts_second_pass_floors(S, exe, exe_chain, tmp, arms):
    import torch
    a = arms("arm7")
    D, n, degree, Wc, B = 7, 8, 3, 100, 256
    ch = S.Chain(a["model"], D, count_static=False)
    P = ch.info()["n_pairs"]
    start, _, _ = TG.free_poses(exe_chain, tmp, a["xml"], D)
    end = W.arm_poses(D, 400, 77, 1.2)[FLOOR_POSE]  # (free_poses' pool)
    knots, c0 = TG.linear_ctrl(S, start, end, n, degree)
    arc = torch.zeros(B, dtype=torch.float64, device="cuda")
    feas = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ctrl = torch.zeros((B, n, D), dtype=torch.float64, device="cuda")
    ch.sample_score(knots, degree, c0, FLOOR_SIGMA, np.full(D, np.pi), Wc, 0, B, arc, feas, S.best_tensor(), ctrl_out=ctrl,
                    seed=FLOOR_SEED)
    torch.cuda.synchronize()
    host = RH.chain(exe, a["xml"], D, waypoints(S, knots, degree, _np(ctrl), Wc).reshape(-1, D), tmp, tag="floors")
    want = RH.path_first(host["contact"].reshape(B, Wc + 1, P))
    wp = want[:, 0]
    counts = (int((wp >= 64).sum()), int(((wp >= 0) & (wp < 64)).sum()), int((wp < 0).sum()))
    print("first contacts (second pass, first pass, none):", counts)
    assert min(counts) >= 8, counts  # from the host alone
    first = _np(ch.first_contacts(knots, degree, ctrl, Wc))
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(first[:, 0] == -1, _np(feas).astype(bool))


# ------------------------------------------------------------------ 4. edges
def spline_args(S, D, n=5, degree=3, B=4):
    knots, c0 = TG.linear_ctrl(S, np.zeros(D), np.full(D, 0.3), n, degree)
    return knots, np.ascontiguousarray(np.tile(c0, (B, 1, 1)))


def test_empty_pair_table(S, tmp):
    """every geom contype = conaffinity = 0: the calls succeed, the outputs are empty, every first record is -1"""
    world = W.capsule_arm_world(3, 21)

    def off(b):
        for g in b.get("geoms", ()):
            g["contype"], g["conaffinity"] = 0, 0
        for c in b.get("children", ()):
            off(c)
    for g in world["geoms"]:
        g["contype"], g["conaffinity"] = 0, 0
    off(world["bodies"][0])
    ch = S.Chain(S.Model(H.write_xml(tmp, "empty", W.mjcf(world)), joints=True), 3, count_static=False)
    assert ch.info()["n_pairs"] == 0 and ch.pairs() == [] and ch.static_pairs() == []
    c, d = ch.pair_contacts(np.zeros((5, 3)))
    assert c.shape == d.shape == (5, 0)
    knots, ctrl = spline_args(S, 3)
    c, d = ch.path_contacts(knots, 3, ctrl, 20)
    assert c.shape == d.shape == (4, 21, 0)
    assert (_np(ch.first_contacts(knots, 3, ctrl, 20)) == -1).all()


def test_single_pair_and_full_table(S, exe, tmp):
    """P = 1, and P = 512 (the largest table: the images of a wave's rows are at their largest)"""
    from sspp_amd import _lib
    for balls in (1, _lib.CHAIN_MAX_PAIRS):
        world = TG.star_world(1, balls)
        # the first ball where the link's sphere swings through it
        world["geoms"][0]["pos"], world["geoms"][0]["size"] = (0.2, 0, 1.0), (0.1, 0, 0)
        xml = H.write_xml(tmp, "balls%d" % balls, W.mjcf(world))
        ch = S.Chain(S.Model(xml, joints=True), 1, count_static=False)
        P = ch.info()["n_pairs"]
        assert P == balls
        q = np.linspace(-2, 2, 131)[:, None]
        host = RH.chain(exe, xml, 1, q, tmp, tag="balls")
        assert (host["contact"][:, 0] > 0).any() and not (host["contact"][:, 0] > 0).all()
        c, d = ch.pair_contacts(q)
        assert _np(c).tobytes() == host["contact"].tobytes() and _np(d).tobytes() == host["deep"].tobytes()
        knots, ctrl = TG.linear_ctrl(S, np.array([-2.0]), np.array([2.0]), 4, 3)
        ctrl = np.ascontiguousarray(np.stack([ctrl, 0.1 * ctrl - 1.5]))
        hp = RH.chain(exe, xml, 1, waypoints(S, knots, 3, ctrl, 70).reshape(-1, 1), tmp, tag="balls_path")
        c, d = ch.path_contacts(knots, 3, ctrl, 70)
        assert _np(c).tobytes() == hp["contact"].tobytes() and _np(d).tobytes() == hp["deep"].tobytes()
        first = _np(ch.first_contacts(knots, 3, ctrl, 70))
        np.testing.assert_array_equal(first, RH.path_first(hp["contact"].reshape(2, 71, P)))
        assert first[0, 0] > 0 and first[0, 1] == 0 and first[1].tolist() == [-1, -1]


def test_job_cache_replaced_and_back(S, exe_chain, tmp, arms):
    """the path forms after a score_ctrl of another shape, and back: the cached job is replaced, the results stay"""
    a = arms("arm7")
    ch = S.Chain(a["model"], 7, count_static=False)
    knots, ctrl = TG.random_splines(S, exe_chain, tmp, a["xml"], 7, 40, 6, 3, 31)
    knots2, ctrl2 = TG.random_splines(S, exe_chain, tmp, a["xml"], 7, 40, 9, 2, 32)
    d = dev(ctrl)
    c0, d0 = ch.path_contacts(knots, 3, d, 50)
    f0 = _np(ch.first_contacts(knots, 3, d, 50))
    _, feas0, _ = TG.run_score(S, ch, knots, 3, ctrl, 50)
    TG.run_score(S, ch, knots2, 2, ctrl2, 33)  # another shape: the job is replaced
    c1, d1 = ch.path_contacts(knots, 3, d, 50)
    TG.run_score(S, ch, knots2, 2, ctrl2, 33)
    f1 = _np(ch.first_contacts(knots, 3, d, 50))
    _, feas1, _ = TG.run_score(S, ch, knots, 3, ctrl, 50)
    assert _np(c0).tobytes() == _np(c1).tobytes() and _np(d0).tobytes() == _np(d1).tobytes()
    assert np.array_equal(f0, f1) and np.array_equal(feas0, feas1) and np.array_equal(f0[:, 0] == -1, feas0)
    assert (f0[:, 0] >= 0).any() and (f0[:, 0] < 0).any()


def test_bad_arguments(S, arms):
    import torch
    from sspp_amd import _lib
    L = _lib.lib()
    a = arms("arm3")
    ch = S.Chain(a["model"], 3, count_static=False)
    P = ch.info()["n_pairs"]
    knots, ctrl = spline_args(S, 3)
    dk = knots.ctypes.data_as(C.POINTER(C.c_double))
    dq = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    dctrl = dev(ctrl)
    out = torch.zeros((4 * 21 * P,), dtype=torch.uint8, device="cuda")
    first = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    n = C.c_int()
    cases = [
        ("null chain", lambda: L.sspp_chain_pair_contacts(None, vp(dq), 4, vp(out), None, None)),
        ("negative pose count", lambda: L.sspp_chain_pair_contacts(ch.handle, vp(dq), -1, vp(out), None, None)),
        ("null poses", lambda: L.sspp_chain_pair_contacts(ch.handle, None, 4, vp(out), None, None)),
        ("null poses / contact", lambda: L.sspp_chain_pair_contacts(ch.handle, vp(dq), 4, None, None, None)),
        ("null chain", lambda: L.sspp_chain_path_contacts(None, dk, 3, vp(dctrl), 4, 5, 20, vp(out), None, None)),
        ("negative path count", lambda: L.sspp_chain_path_contacts(ch.handle, dk, 3, vp(dctrl), -1, 5, 20, vp(out), None, None)),
        ("null paths", lambda: L.sspp_chain_path_contacts(ch.handle, dk, 3, None, 4, 5, 20, vp(out), None, None)),
        ("null paths / contact", lambda: L.sspp_chain_path_contacts(ch.handle, dk, 3, vp(dctrl), 4, 5, 20, None, None, None)),
        ("null knots", lambda: L.sspp_chain_path_contacts(ch.handle, None, 3, vp(dctrl), 4, 5, 20, vp(out), None, None)),
        ("check_points", lambda: L.sspp_chain_path_contacts(ch.handle, dk, 3, vp(dctrl), 4, 5, -2, vp(out), None, None)),
        ("check_points", lambda: L.sspp_chain_path_contacts(ch.handle, dk, 3, vp(dctrl), 4, -5, 20, vp(out), None, None)),
        ("null chain", lambda: L.sspp_chain_first_contacts(None, dk, 3, vp(dctrl), 4, 5, 20, vp(first), None)),
        ("negative path count", lambda: L.sspp_chain_first_contacts(ch.handle, dk, 3, vp(dctrl), -4, 5, 20, vp(first), None)),
        ("null output", lambda: L.sspp_chain_first_contacts(ch.handle, dk, 3, vp(dctrl), 4, 5, 20, None, None)),
        ("null paths", lambda: L.sspp_chain_first_contacts(ch.handle, dk, 3, None, 4, 5, 20, vp(first), None)),
        ("check_points", lambda: L.sspp_chain_first_contacts(ch.handle, dk, 3, vp(dctrl), 4, 5, 0, vp(first), None)),
        # more than 2^31 - 1 workgroups: refused before anything is launched
        ("too many poses", lambda: L.sspp_chain_pair_contacts(ch.handle, vp(dq), 2 ** 38, vp(out), None, None)),
        ("too many poses", lambda: L.sspp_chain_path_contacts(ch.handle, dk, 3, vp(dctrl), 2 ** 38, 5, 20, vp(out), None, None)),
        ("too many paths", lambda: L.sspp_chain_first_contacts(ch.handle, dk, 3, vp(dctrl), 2 ** 31, 5, 20, vp(first), None)),
        ("null argument", lambda: L.sspp_chain_static_pairs(None, None, None, None, 0, C.byref(n))),
        ("null argument", lambda: L.sspp_chain_static_pairs(ch.handle, None, None, None, 0, None)),
        ("bad argument", lambda: L.sspp_chain_pair_contacts_host(None, None, 4, None, None)),
        ("bad argument", lambda: L.sspp_chain_path_contacts_host(ch.handle, dk, 3, None, -1, 5, 20, None, None)),
        ("bad argument", lambda: L.sspp_chain_first_contacts_host(ch.handle, dk, 3, None, 4, 5, -1, None)),
    ]
    for msg, call in cases:
        assert call() == -1, msg
        assert msg in _lib.last_error(), (msg, _lib.last_error())
    # a degree the planner does not have is unsupported, as for score_ctrl
    assert L.sspp_chain_path_contacts(ch.handle, dk, 4, vp(dctrl), 4, 5, 20, vp(out), None, None) == -5
    # nothing to do is not an error, whatever the pointers
    assert L.sspp_chain_pair_contacts(ch.handle, None, 0, None, None, None) == 0
    assert L.sspp_chain_path_contacts(ch.handle, None, 3, None, 0, 5, 20, None, None, None) == 0
    assert L.sspp_chain_first_contacts(ch.handle, None, 3, None, 0, 5, 20, None, None) == 0


def test_host_forms(S, arms):
    """the _host forms on numpy buffers equal the device forms"""
    from sspp_amd import _lib
    L = _lib.lib()
    a = arms("arm7")
    ch = S.Chain(a["model"], 7, count_static=False)
    P = ch.info()["n_pairs"]
    q = W.arm_poses(7, 70, 9, 2.0)
    knots, c0 = TG.linear_ctrl(S, q[0], q[1], 6, 3)
    ctrl = np.ascontiguousarray(np.stack([c0, 0.5 * c0, 0.1 * c0]))
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    bp = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))   # noqa: E731
    c, d = np.full((70, P), 9, np.uint8), np.full((70, P), 9, np.uint8)
    _lib.check(L.sspp_chain_pair_contacts_host(ch.handle, dp(q), 70, bp(c), bp(d)), "pair_contacts_host")
    gc, gd = ch.pair_contacts(q)
    assert c.tobytes() == _np(gc).tobytes() and d.tobytes() == _np(gd).tobytes() and (c > 0).any()
    c, d = np.full((3, 41, P), 9, np.uint8), np.full((3, 41, P), 9, np.uint8)
    _lib.check(L.sspp_chain_path_contacts_host(ch.handle, dp(knots), 3, dp(ctrl), 3, 6, 40, bp(c), bp(d)), "path_contacts_host")
    gc, gd = ch.path_contacts(knots, 3, ctrl, 40)
    assert c.tobytes() == _np(gc).tobytes() and d.tobytes() == _np(gd).tobytes()
    c2 = np.full((3, 41, P), 9, np.uint8)
    _lib.check(L.sspp_chain_path_contacts_host(ch.handle, dp(knots), 3, dp(ctrl), 3, 6, 40, bp(c2), None), "path_contacts_host")
    assert c2.tobytes() == c.tobytes()
    first = (_lib.ChainFirst * 3)()
    _lib.check(L.sspp_chain_first_contacts_host(ch.handle, dp(knots), 3, dp(ctrl), 3, 6, 40, first), "first_contacts_host")
    got = np.array([(f.waypoint, f.pair) for f in first], np.int32)
    np.testing.assert_array_equal(got, _np(ch.first_contacts(knots, 3, ctrl, 40)))
    np.testing.assert_array_equal(got, RH.path_first(c))
    assert C.sizeof(_lib.ChainFirst) == 8


def test_live_resources_flat(S, arms):
    """20 repeated calls of each form allocate nothing that stays"""
    a = arms("arm7")
    ch = S.Chain(a["model"], 7, count_static=False)
    q = dev(W.arm_poses(7, 100, 9, 2.0))
    knots, ctrl = spline_args(S, 7, n=6, B=10)
    dctrl = dev(ctrl)

    def once():
        ch.pair_contacts(q)
        ch.path_contacts(knots, 3, dctrl, 30)
        ch.first_contacts(knots, 3, dctrl, 30)
        ch.static_pairs()

    once()  # (the first call of the shape makes the job)
    before = live_resources()
    for _ in range(20):
        once()
    assert live_resources() == before
