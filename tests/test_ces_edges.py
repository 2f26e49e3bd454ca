"""The CES update kernels, the TaskSpacePlanner sampler and the many-via evaluation on crafted
inputs the shipped scenes never produce (cases: tests/ces_edge_cases.py).

Injection route: set_state -> begin(iterate=True) -> sspp_ces_unpack of packed records the test
wrote -> update -> read runs k_ces_rank / k_ces_scatter / k_ces_update (or the fused one-launch
update) on exactly the list a test chose, with no evaluation in between.  Bars, as in
tests/test_ces.py: read() returns the injected per-slot arrays bit for bit; success and elite
counts, elites, best slot and cost, has_best, mean, sigma and last best bit-identical to
O.ces_update in the canonical summation order.  The CPU tests check every crafted list on the
oracle alone against the literal restatement of the reference (sequential order bit-equal,
canonical order <= 1e-12) and that each case reaches the branch it is named for.

Sampler: device samples against O.sample_tsp at max |delta| <= 1e-12, 4096 samples per case,
through the CES slot mode and through TspJob.sample_score.  On the MI355X every case of both
routes was bit-identical to the oracle (max |delta| = 0).

Many vias (K = 8, 32, 60; 96 candidates; 40 and 65 check points): status equal; costs within a bar
that is not fixed in advance but measured on the CPU: the oracle's relative deviation, in both of
its summation orders, from a np.longdouble restatement of the interpolation and arc length
(ces_edge_cases.arc_length_longdouble), times 16 (the device replays the QR solve in a different
but equally valid operation order), floored at 1e-12 relative.  Measured: the deviations are
7.4e-16 .. 1.0e-15 (K = 8), 1.5e-15 .. 1.6e-15 (K = 32) and 1.9e-15 .. 2.3e-15 (K = 60), so
16 x 2.3e-15 = 3.7e-14 stays under the floor and the bar is 1e-12 relative for every case.

A NaN cost is kept out of every list: the reference's partial_sort on NaN is undefined, the
device treats a NaN-cost success as a non-success and the oracle counts it (CES).
"""
import functools
import os

import numpy as np
import pytest

from oracle import mjcf_ref
from oracle import oracle as O
from tests import ces_edge_cases as E
from tests.conftest import SCENES
from tests.test_ces import literal_update

STACKING = os.path.join(SCENES, "stacking.xml")
SEED = 0x5EED
UPDATE = E.update_cases()
SEQUENCES = {c["id"]: c for c in (E.rearm_case(), E.padding_case())}
ALL_LISTS = dict(UPDATE, **SEQUENCES)
SAMPLER = E.sampler_cases()
NS = 4096
# the elite count each named case must reach (int(nsucc * frac) in double, at least 1)
EXPECT_K = {"k1": 1, "k2": 2, "k511": 511, "k512": 512, "k513": 513, "k1024": 1024, "k1025": 1025,
            "k8192": 8192, "round_100_0.29": 28, "round_100_0.57": 56, "round_100_0.07": 7,
            "round_10_0.3": 3, "round_7_0.3": 2, "round_3_0.0": 1}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def oracle_chain(case):
    """O.ces_update over the case's lists in the canonical order, state carried from list to list:
    [(state_in, result)], state = (mean, sigma, last_best, has_best)."""
    state = (case["mean"], case["sigma"], case["lbest"], True)
    out = []
    for lst in case["lists"]:
        m, s, lb, hb, ns, el, bs = O.ces_update(lst["cost"], lst["status"], lst["vias"], *state, **case["cfg"])
        out.append((state, dict(mean=m, sigma=s, last_best=lb, has_best=hb, n_success=ns, elites=el,
                                best_slot=bs)))
        state = (m, s, lb, hb)
    return out


# ------------------------------------------------------------------ CPU: the cases on the oracle
@pytest.mark.parametrize("cid", sorted(ALL_LISTS))
def test_oracle_matches_literal_reference_on_crafted_lists(cid):
    case = ALL_LISTS[cid]
    cfg = case["cfg"]
    for lst, (state, can) in zip(case["lists"], oracle_chain(case)):
        m0, s0, lb0, hb0 = state
        cost, status, vias = lst["cost"], lst["status"], lst["vias"]
        assert np.isfinite(vias).all() and not np.isnan(cost).any()
        lit_s, lit_m, lit_best, lit_el = literal_update(cost, status, vias, m0, s0, **cfg)
        m, s, lb, hb, ns, el, bs = O.ces_update(cost, status, vias, m0, s0, lb0, hb0, sequential=True, **cfg)
        assert ns == can["n_success"] == int(status.sum())
        assert list(el) == list(can["elites"]) == lit_el
        assert bs == can["best_slot"] == (-1 if lit_best is None else lit_best)
        np.testing.assert_array_equal(bits(m), bits(np.array(lit_m)))  # sequential: bit-equal
        np.testing.assert_array_equal(bits(s), bits(np.array(lit_s)))
        assert np.abs(can["mean"] - np.array(lit_m)).max() <= 1e-12      # canonical order
        assert np.abs(can["sigma"] - np.array(lit_s)).max() <= 1e-12
        if ns == 0:
            assert hb and can["has_best"]  # the forwarded best stays
            np.testing.assert_array_equal(bits(can["last_best"]), bits(lb0))
            np.testing.assert_array_equal(bits(can["mean"]), bits(m0))
        else:
            np.testing.assert_array_equal(bits(can["last_best"]), bits(vias[lit_best]))
    key = cid.rsplit("_n", 1)[0] if cid.startswith("round_") else cid
    if key in EXPECT_K:
        assert len(oracle_chain(case)[0][1]["elites"]) == EXPECT_K[key]


def test_crafted_lists_reach_their_branches():
    """What the case names promise, checked on the data and the oracle alone."""
    assert sorted({UPDATE["size%d" % n]["n"] for n in (3, 64, 65, 256, 257, 512, 513, 1025)}) == [
        3, 64, 65, 256, 257, 512, 513, 1025]
    for n in (257, 513, 1025):  # equal-cost runs across the tile borders, inside the elite set
        c = UPDATE["size%d" % n]
        lst, el = c["lists"][0], list(oracle_chain(c)[0][1]["elites"])
        assert lst["cost"][254] == lst["cost"][255] == lst["cost"][256] and lst["status"][253:257].all()
        assert el.index(254) + 1 == el.index(255) and el.index(255) + 1 == el.index(256)
        if n > 257:
            assert lst["cost"][257] == lst["cost"][256] and el.index(256) + 1 == el.index(257)
        if n > 513:
            assert el.index(511) + 1 == el.index(512) and el.index(512) + 1 == el.index(513)
    for n in (300, 513):        # all costs equal: the elites are the lowest slots, in order
        el = oracle_chain(UPDATE["equal%d" % n])[0][1]["elites"]
        assert list(el) == list(range(len(el))) and len(el) == int(n * 0.3)
    for n in (64, 300):         # -0 and +0 compare equal: slot order decides among them
        c = UPDATE["zeros%d" % n]
        cost, el = c["lists"][0]["cost"], oracle_chain(c)[0][1]["elites"]
        sg = np.signbit(cost[el])
        assert sg.any() and not sg.all() and (np.diff(el) > 0).all()
    for n in (64, 600):
        c = UPDATE["negative%d" % n]["lists"][0]
        assert (c["cost"][c["status"] == 1] < 0).any()
    for n in (6, 300):          # a +inf success is an elite (frac 1), and the last one
        c = UPDATE["inf%d" % n]
        el = oracle_chain(c)[0][1]["elites"]
        assert list(el[-2:]) == [1, n - 2] and np.isinf(c["lists"][0]["cost"][el[-1]])
    for n in (64, 600):         # mean clamps: x at hi, y at lo, z at dist_z_min
        c = UPDATE["meanclamp%d" % n]
        m = oracle_chain(c)[0][1]["mean"]
        assert (m[:, 0] == c["cfg"]["hi"][0]).all() and (m[:, 1] == c["cfg"]["lo"][1]).all()
        assert (m[:, 2] == c["cfg"]["dist_z_min"]).all()
        c = UPDATE["floor%d" % n]
        assert (oracle_chain(c)[0][1]["sigma"] == 0.7).all()
        assert (oracle_chain(UPDATE["floor_none%d" % n])[0][1]["sigma"] == 0.7).all()
        s = oracle_chain(UPDATE["sigmaedges_none%d" % n])[0][1]["sigma"][0]
        assert list(s) == [0.01 * 1.5, 0.5, 0.01, 0.2 * 1.5]
        c = UPDATE["beta0_lr0_n%d" % n]  # beta 0, lr 0: mean kept (inside the bounds), sigma decays
        r = oracle_chain(c)[0][1]
        np.testing.assert_array_equal(r["mean"], c["mean"])
    # yaw: the wrapped differences decide a sigma that no clamp hides; a narrow range takes > 10 turns
    for cid in ("seam6", "seam6_keep", "seam64", "seam700", "narrowyaw64", "narrowyaw700"):
        c = UPDATE[cid]
        sy = oracle_chain(c)[0][1]["sigma"][:, 3]
        assert ((sy > c["cfg"]["sd_min"]) & (sy < 0.95 * c["cfg"]["sd_max"])).all(), cid
    assert (oracle_chain(UPDATE["seam6_keep"])[0][1]["sigma"][:, 3] < 0.15).all()
    for n in (64, 700):
        lst = UPDATE["narrowyaw%d" % n]["lists"][0]
        assert np.abs(lst["vias"][lst["status"] == 1, 0, 3]).max() > 10 * 0.2
        assert np.abs(lst["vias"][..., 3]).max() < 40 * 0.2
    r = [x[1] for x in oracle_chain(SEQUENCES["rearm"])]
    assert [x["n_success"] for x in r] == [600, 17, 0, 600] and [len(x["elites"]) for x in r] == [600, 17, 0, 600]


@functools.lru_cache(maxsize=None)
def sampler_oracle(sid):
    c = SAMPLER[sid]
    return O.sample_tsp(c["mean"], c["sigma"], c["lo"], c["hi"], c["z_min"], SEED, 0, NS, with_tries=True)


def test_sampler_cases_reach_both_outcomes():
    for i in range(3):
        v, t = sampler_oracle("degenerate%d" % i)
        assert (t[:, :, i] == 0).all() and (v[:, :, i] == SAMPLER["degenerate%d" % i]["lo"][i]).all()
        assert (t[:, :, [j for j in range(3) if j != i]] > 0).all()
        v, t = sampler_oracle("narrow%d" % i)
        acc = (t[:, 0, i] > 0).mean()
        assert 0.05 <= acc <= 0.95, acc  # both the accepted draw and the 99-miss fallback occur
        assert (t[:, 0, i] > 50).sum() > 0
        c = SAMPLER["narrow%d" % i]
        assert ((v[:, 0, i] >= c["lo"][i]) & (v[:, 0, i] <= c["hi"][i])).all()
        v, t = sampler_oracle("meanonbound%d" % i)
        assert 0.3 < (t[:, 0, i] > 1).mean() < 0.7 and (t[:, 0, i] > 0).all()
    c = SAMPLER["zclamp"]
    v, t = sampler_oracle("zclamp")
    clamped = v[:, 0, 2] == c["z_min"]
    assert clamped.sum() > 100 and (~clamped).sum() > 100 and (t[clamped, 0, 2] > 0).all()
    assert (v[:, 0, 2] >= c["z_min"]).all()
    c = SAMPLER["yaw_many_wraps"]  # raw draw = z0 * sigma + mean, several ranges outside the bounds
    v, _ = sampler_oracle("yaw_many_wraps")
    raw = np.array([O.normal_pair(SEED, g, 3 << 7, 1)[0] for g in range(512)]) * c["sigma"][0, 3] + c["mean"][0, 3]
    assert (np.abs(raw) > 0.05 + 2 * 0.1).mean() > 0.3
    assert (np.abs(v[:, 0, 3]) <= 0.05).all()
    assert np.abs(np.remainder(raw - v[:512, 0, 3] + 0.05, 0.1) - 0.05).max() < 1e-9
    v, _ = sampler_oracle("yaw_mean_on_hi")
    assert (v[:, 0, 3] < 0).mean() > 0.3  # draws above hi wrap to the lower end
    v, _ = sampler_oracle("yaw_fixed")
    assert (v[:, 0, 3] == 0.2).all()      # lo[3] == hi[3]: the mean's yaw, no draw
    assert SAMPLER["vias32"]["K"] == 32


# ------------------------------------------------------------------ many vias: cases and the bar
MV_START, MV_END = np.array([0.205, 0.0, 0.30, 0.0]), np.array([0.0, 0.0, 0.42, 0.3])
MV_B = 96
MV_KS = (8, 32, 60)
MV_CPS = (40, 65)


@functools.lru_cache(maxsize=None)
def stacking_oracle_scene():
    import sspp_amd as S
    body = S.Model(STACKING).body_id("block1")
    return O.Scene(mjcf_ref.load(STACKING), 1, body)


@functools.lru_cache(maxsize=None)
def many_via_case(K, cp):
    """Via sets, the oracle's results and the device bar of one (K, check points) case."""
    v = E.via_sets(K, MV_B, MV_START, MV_END, 100 + K, dip=0.25)
    osc = stacking_oracle_scene()
    L, Cnf, Cwf, st, cost = O.tsp_score(osc, MV_START, MV_END, v, cp)
    Lseq = O.tsp_score(osc, MV_START, MV_END, v, cp, sequential=True)[0]
    Lld = E.arc_length_longdouble(MV_START, MV_END, v, cp)
    dev = max(float(np.abs((L - Lld) / Lld).max()), float(np.abs((Lseq - Lld) / Lld).max()))
    return dict(vias=v, L=L, C_nf=Cnf, C_wf=Cwf, status=st, cost=cost, dev=dev, bar=max(1e-12, 16.0 * dev))


@pytest.mark.parametrize("K", MV_KS)
@pytest.mark.parametrize("cp", MV_CPS)
def test_many_via_cases_on_the_oracle(K, cp):
    c = many_via_case(K, cp)
    print("K %d cp %d: %d / %d successes, oracle vs longdouble %.3g relative, device bar %.3g"
          % (K, cp, int(c["status"].sum()), MV_B, c["dev"], c["bar"]))
    assert c["status"].sum() >= 1 and (c["status"] == 0).sum() >= 1
    assert c["dev"] <= 1e-13  # two independent restatements agree to rounding
    assert np.isfinite(c["cost"][c["status"] == 1]).all()


def test_ces_34_points_case_has_successes():
    recs = O.ces_plan(stacking_oracle_scene(), MV_START, MV_END, iterations=2, samples=100, checks=40,
                      total_points=34, **CES34)
    assert all(0 < r["n_success"] < 101 for r in recs)


CES34 = dict(sd_min=0.001, sd_max=0.004, lo=E.LO, hi=E.HI)


# ------------------------------------------------------------------ device
@pytest.fixture(scope="module")
def stk(cuda):
    import sspp_amd as S
    model = S.Model(STACKING)
    body = model.body_id("block1")
    return dict(S=S, model=model, scene=S.Scene(model, 1, body), osc=stacking_oracle_scene())


def make_planner(stk, case, world=1, fused=1):
    S = stk["S"]
    pl = S.CesPlanner(stk["scene"], seed=SEED, world=world, rank=0, **E.planner_kwargs(case))
    if not fused:
        pl.set_option(S.OPT_CES_FUSED, 0)
    return pl


def inject(pl, lst, state=None):
    """begin(iterate=True) with a forwarded best (n_fixed = 2: every slot live), the crafted
    records unpacked into the planner, update, read.  state: (mean, sigma, last_best) to set
    first; None keeps the device's own."""
    import torch
    from sspp_amd._lib import lib
    from sspp_amd.runtime import _ptr, _stream
    if state is not None:
        pl.set_state(state[0], state[1], state[2], has_best=1)
    pl.begin(E.START, E.END, iterate=True)
    rec = torch.from_numpy(E.pack(lst, pl.n_slots, pl.K)).cuda()
    assert lib().sspp_ces_unpack(pl._h, _ptr(rec), _stream(None)) == 0
    pl.update()
    return pl.read()


def check_update(r, lst, want, tag=""):
    n = len(lst["cost"])
    assert r["n_fixed"] == 2 and r["n_candidates"] == n, tag
    for k in ("L", "C_nf", "C_wf", "cost", "vias"):
        np.testing.assert_array_equal(bits(r[k]), bits(lst[k]), err_msg="%s %s" % (tag, k))
    np.testing.assert_array_equal(r["status"], lst["status"], err_msg=tag)
    assert r["n_success"] == want["n_success"] and r["n_elite"] == len(want["elites"]), tag
    np.testing.assert_array_equal(r["elites"], want["elites"], err_msg=tag)
    assert r["best_slot"] == want["best_slot"] and r["has_best"] == want["has_best"], tag
    bc = np.inf if want["best_slot"] < 0 else lst["cost"][want["best_slot"]]
    assert bits(r["best_cost"]) == bits(bc), tag
    for k in ("mean", "sigma", "last_best"):
        np.testing.assert_array_equal(bits(r[k]), bits(want[k]), err_msg="%s %s" % (tag, k))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(UPDATE))
def test_update_kernels_on_injected_lists(stk, cid):
    case = UPDATE[cid]
    (state, want), = oracle_chain(case)
    for fused in ((1, 0) if case["n"] <= 512 else (1,)):
        pl = make_planner(stk, case, fused=fused)
        assert pl.n_slots == case["n"]
        r = inject(pl, case["lists"][0], state[:3])
        check_update(r, case["lists"][0], want, "%s fused=%d" % (cid, fused))


@pytest.mark.gpu
def test_elite_capacity_boundary(stk):
    """(samples + 2) * elite_fraction == 8192 is the largest list of elites (the k8192 case runs
    it); one more is refused at creation."""
    S = stk["S"]
    S.CesPlanner(stk["scene"], sample_count=8190, check_points=8, elite_fraction=1.0)
    with pytest.raises(S.SsppError, match="8192"):
        S.CesPlanner(stk["scene"], sample_count=8191, check_points=8, elite_fraction=1.0)


@pytest.mark.gpu
def test_rank_and_success_counter_rearmed_between_updates(stk):
    case = SEQUENCES["rearm"]
    pl = make_planner(stk, case)
    for t, (lst, (state, want)) in enumerate(zip(case["lists"], oracle_chain(case))):
        r = inject(pl, lst, state[:3] if t == 0 else None)  # later updates: the device's own state
        check_update(r, lst, want, "update %d" % t)
        assert r["iteration"] == t + 1


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_padded_slots_do_not_count(stk, world):
    case = SEQUENCES["padding"]
    lst = case["lists"][0]
    (state, want), = oracle_chain(case)
    single = inject(make_planner(stk, case), lst, state[:3])
    pl = make_planner(stk, case, world=world)
    assert pl.n_slots == 102 > case["n"]
    r = inject(pl, lst, state[:3])
    check_update(r, lst, want)
    for k in single:
        np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(single[k]), err_msg=k)


@pytest.mark.gpu
def test_pack_unpack_round_trip_is_bit_exact(stk):
    import torch
    from sspp_amd._lib import lib
    from sspp_amd.runtime import _ptr, _stream
    lst = E.special_list()
    n, K = len(lst["cost"]), lst["vias"].shape[1]
    case = E.case("roundtrip", n, K=K, lists=[lst])
    pl = make_planner(stk, case)
    rec = E.pack(lst, pl.n_slots, K)
    assert np.signbit(rec[rec == 0]).any() and np.isinf(rec).any() and ((rec != 0) & (np.abs(rec) < 1e-300)).any()
    din = torch.from_numpy(rec).cuda()
    dout = torch.zeros_like(din)
    assert lib().sspp_ces_unpack(pl._h, _ptr(din), _stream(None)) == 0
    assert lib().sspp_ces_pack(pl._h, 0, _ptr(dout), _stream(None)) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(dout.cpu().numpy()), bits(rec))


# ---- sampler
def sampler_diff(got, sid):
    want, _ = sampler_oracle(sid)
    d = float(np.abs(got - want).max())
    print("sampler %s: max |delta| %.3g, bit-identical %s" % (sid, d, np.array_equal(bits(got), bits(want))))
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("sid", sorted(SAMPLER))
def test_sampler_in_ces_slot_mode(stk, sid):
    c = SAMPLER[sid]
    S = stk["S"]
    pl = S.CesPlanner(stk["scene"], sample_count=NS, check_points=8, init_points=c["K"] + 2, seed=SEED,
                      limits_min=c["lo"], limits_max=c["hi"], z_min=c["z_min"])
    pl.set_state(c["mean"], c["sigma"], np.zeros((c["K"], 4)), has_best=0)
    pl.begin(E.START, E.END, iterate=True)
    pl.eval()
    r = pl.read()
    assert r["n_fixed"] == 1 and r["n_candidates"] == NS + 1
    m = c["mean"]
    np.testing.assert_array_equal(r["vias"][0], np.where(np.arange(4) == 2, np.maximum(m, c["z_min"]), m))
    assert sampler_diff(r["vias"][1:], sid) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("sid", sorted(SAMPLER))
def test_sampler_through_sample_score(stk, sid):
    import torch
    c = SAMPLER[sid]
    job = stk["S"].TspJob(stk["scene"], E.START, E.END, c["K"], 8, mean=c["mean"], sigma=c["sigma"], lo=c["lo"],
                          hi=c["hi"], z_min=c["z_min"], seed=SEED, max_batch=NS)
    o = job.alloc(NS, with_vias=True)
    job.sample_score(0, NS, o["L"], o["Cnf"], o["Cwf"], o["status"], o["cost"], o["best"], vias_out=o["vias"])
    torch.cuda.synchronize()
    assert sampler_diff(o["vias"].cpu().numpy(), sid) <= 1e-12


# ---- many vias
def close(a, b, bar):
    return (np.abs(a - b) <= bar * np.maximum(1.0, np.abs(b))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [-1, 0])
@pytest.mark.parametrize("cp", MV_CPS)
@pytest.mark.parametrize("K", MV_KS)
def test_score_many_vias(stk, K, cp, form):
    import torch
    S = stk["S"]
    c = many_via_case(K, cp)
    job = S.TspJob(stk["scene"], MV_START, MV_END, K, cp, lo=E.LO, hi=E.HI, seed=SEED, max_batch=MV_B)
    if form >= 0:
        job.set_option(S.OPT_TSP_FORM, form)
    o = job.alloc(MV_B)
    job.score_vias(torch.from_numpy(c["vias"]).cuda(), 0, o["L"], o["Cnf"], o["Cwf"], o["status"], o["cost"],
                   o["best"])
    torch.cuda.synchronize()
    got = {k: o[k].cpu().numpy() for k in ("L", "Cnf", "Cwf", "status", "cost")}
    np.testing.assert_array_equal(got["status"], c["status"])
    fin = np.isfinite(c["cost"])
    np.testing.assert_array_equal(np.isfinite(got["cost"]), fin)
    for a, b in ((got["cost"][fin], c["cost"][fin]), (got["L"], c["L"]), (got["Cnf"], c["C_nf"]),
                 (got["Cwf"], c["C_wf"])):
        rel = np.abs(a - b) / np.maximum(1.0, np.abs(b))
        print("K %d cp %d form %d: max relative deviation %.3g (bar %.3g)" % (K, cp, form, rel.max(), c["bar"]))
        assert close(a, b, c["bar"])
    idx = S.decode_best(o["best"])[1]
    assert idx == O.tsp_best(c["cost"], c["status"])[0]


@pytest.mark.gpu
def test_largest_via_count_is_60(stk):
    """sspp_job_create_tsp takes 0..60 via points (test_score_many_vias runs 60); 61 is refused."""
    S = stk["S"]
    with pytest.raises(S.SsppError, match="n_vias"):
        S.TspJob(stk["scene"], MV_START, MV_END, 61, 40, lo=E.LO, hi=E.HI, max_batch=8)


@pytest.mark.gpu
def test_ces_iterations_with_34_points(stk):
    """init_points = 34 (32 vias, the most sspp_ces_create takes; k_ces_begin's 128 threads all
    busy): two iterations, each against the oracle as test_device_ces_matches_oracle_each_iteration."""
    S = stk["S"]
    samples, checks, K = 100, 40, 32
    pl = S.CesPlanner(stk["scene"], sample_count=samples, check_points=checks, init_points=34, seed=SEED,
                      limits_min=E.LO, limits_max=E.HI, stddev_min=CES34["sd_min"], stddev_max=CES34["sd_max"])
    with pytest.raises(S.SsppError, match="total_points"):
        S.CesPlanner(stk["scene"], sample_count=samples, check_points=checks, init_points=35)
    cfg = dict(sd_min=CES34["sd_min"], sd_max=CES34["sd_max"], lo=E.LO, hi=E.HI)
    m_in, s_in = O.ces_reset(MV_START, MV_END, 34, sd_min=cfg["sd_min"], sd_max=cfg["sd_max"], lo=E.LO, hi=E.HI)
    lb_in, hb_in = np.zeros((K, 4)), False
    for t in range(2):
        pl.step(MV_START, MV_END, iterate=t > 0)
        r = pl.read()
        nfx = 2 if (t > 0 and hb_in) else 1
        assert r["n_fixed"] == nfx and r["n_candidates"] == nfx + samples
        np.testing.assert_array_equal(r["vias"][0], np.where(np.arange(4) == 2, np.maximum(m_in, 0.0), m_in))
        if nfx == 2:
            np.testing.assert_array_equal(r["vias"][1], lb_in)
        smp = O.sample_tsp(m_in, s_in, E.LO, E.HI, 0.0, SEED, t * samples, samples)
        assert np.abs(r["vias"][nfx:] - smp).max() <= 1e-12
        L, Cnf, Cwf, st, cost = O.tsp_score(stk["osc"], MV_START, MV_END, r["vias"], checks)
        np.testing.assert_array_equal(r["status"], st)
        for a, b in ((r["L"], L), (r["C_nf"], Cnf), (r["C_wf"], Cwf), (r["cost"], cost)):
            assert np.abs(a - b).max() <= 1e-9
        m, s, lb, hb, ns, el, bs = O.ces_update(r["cost"], r["status"], r["vias"], m_in, s_in, lb_in, hb_in, **cfg)
        assert r["n_success"] == ns > 0 and r["best_slot"] == bs and r["has_best"] == hb
        np.testing.assert_array_equal(r["elites"], el)
        np.testing.assert_array_equal(r["mean"], m)
        np.testing.assert_array_equal(r["sigma"], s)
        np.testing.assert_array_equal(r["last_best"], lb)
        m_in, s_in, lb_in, hb_in = m, s, lb, hb


# ---- lifecycle
@pytest.mark.gpu
@pytest.mark.parametrize("n", [66, 600])
def test_reset_after_a_full_list_drops_the_last_slot(stk, n):
    """An iteration with a forwarded best uses all samples + 2 slots; after begin(iterate=False)
    the list is one shorter and the stale last slot (here the previous list's best) is padding."""
    lst = E.make_list(85, n, 1, "all", cost="cont")
    lst["cost"][-1] = -5.0
    case = E.case("full", n, lists=[lst], seed=85)
    (state, want), = oracle_chain(case)
    pl = make_planner(stk, case)
    r = inject(pl, lst, state[:3])
    check_update(r, lst, want)
    assert r["best_slot"] == n - 1
    start, end = np.array(E.START), np.array(E.END)
    pl.step(start, end, iterate=False)
    r = pl.read()
    assert r["n_fixed"] == 1 and r["n_candidates"] == n - 1
    m0, s0 = O.ces_reset(start, end, 3, lo=E.LO, hi=E.HI)
    m, s, lb, hb, ns, el, bs = O.ces_update(r["cost"], r["status"], r["vias"], m0, s0, np.zeros((1, 4)), False,
                                            **case["cfg"])
    assert 0 < ns == r["n_success"] and r["best_slot"] == bs != n - 1 and r["has_best"] == hb
    np.testing.assert_array_equal(r["elites"], el)
    assert (r["elites"] < n - 1).all()
    for k, w in (("mean", m), ("sigma", s), ("last_best", lb)):
        np.testing.assert_array_equal(bits(r[k]), bits(w), err_msg=k)


@pytest.mark.gpu
def test_set_state(stk):
    S = stk["S"]
    start, end = np.array(E.START), np.array(E.END)
    pl = S.CesPlanner(stk["scene"], sample_count=60, check_points=40, seed=SEED, limits_min=E.LO, limits_max=E.HI)
    assert pl.n_slots <= 512  # the fused update stages read()'s buffer itself
    pl.step(start, end, iterate=False)
    r0 = pl.read()
    mean = np.array([[0.11, -0.07, 0.45, 0.3]])
    pl.set_state(mean=mean)  # has_best = -1: the flag stays
    r1 = pl.read()
    np.testing.assert_array_equal(r1["mean"], mean)  # not the staged copy of the iteration
    assert r1["has_best"] == r0["has_best"]
    np.testing.assert_array_equal(r1["sigma"], r0["sigma"])
    np.testing.assert_array_equal(r1["last_best"], r0["last_best"])
    for flag in (1, 0):
        pl.set_state(has_best=flag)
        assert pl.read()["has_best"] == bool(flag)
        pl.set_state(sigma=np.full((1, 4), 0.05))
        assert pl.read()["has_best"] == bool(flag)
    lbest = np.array([[0.02, 0.03, 0.5, -0.4]])
    sigma = np.array([[0.05, 0.06, 0.07, 0.08]])
    pl.set_state(mean, sigma, lbest, has_best=1)
    pl.begin(start, end, iterate=True)
    pl.eval()
    r = pl.read()
    assert r["n_fixed"] == 2 and r["n_candidates"] == 62
    np.testing.assert_array_equal(r["vias"][0], mean)
    np.testing.assert_array_equal(r["vias"][1], lbest)
    smp = O.sample_tsp(mean, sigma, E.LO, E.HI, 0.0, SEED, 60, 60)  # second evaluation's ids
    assert np.abs(r["vias"][2:] - smp).max() <= 1e-12


GROUP_BOUNDS = {"flat_z": ((-0.5, -0.5, 0.35, -1.6), (0.5, 0.5, 0.35, 1.6)),
                "seam": (E.PI_LO, E.PI_HI)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(GROUP_BOUNDS))
def test_plan_group_from_set_states(stk, which):
    """sspp_ces_plan_group (k_ces_begin_group, k_tsp_group, k_ces_update_group) continuing four
    planners whose distributions set_state wrote: degenerate z bounds (every z is the fallback)
    and means on the +-pi yaw seam.  Per goal against the oracle, as
    test_ces_plan_group_matches_oracle."""
    S = stk["S"]
    lo, hi = GROUP_BOUNDS[which]
    samples, checks, G = 70, 65, 4
    rng = np.random.default_rng(91)
    starts = np.array(E.START) + np.array([0.0, 0.0, 0.23, 0.0]) + 0.02 * rng.standard_normal((G, 4))
    ends = np.array(E.END) + np.array([0.0, 0.0, 0.1, 0.0]) + 0.02 * rng.standard_normal((G, 4))
    pls, states = [], []
    for g in range(G):
        pl = S.CesPlanner(stk["scene"], sample_count=samples, check_points=checks, seed=SEED + g,
                          limits_min=lo, limits_max=hi)
        mean = np.array([[0.1 - 0.05 * g, 0.02 * g, 0.35, (3.1, -3.12, 3.14, -3.0)[g] if which == "seam" else 0.2 * g]])
        sigma = np.array([[0.02, 0.03, 0.04, 0.2 + 0.05 * g]])
        lbest = mean + 0.01
        pl.set_state(mean, sigma, lbest, has_best=g % 2)
        pls.append(pl)
        states.append((mean, sigma, lbest, bool(g % 2)))
    S.CesPlanner.plan_group(pls, starts, ends, iterate=True, iterations=1)
    succ = 0
    for g, pl in enumerate(pls):
        m_in, s_in, lb_in, hb_in = states[g]
        r = pl.read()
        nfx = 2 if hb_in else 1
        assert r["n_fixed"] == nfx and r["n_candidates"] == nfx + samples
        np.testing.assert_array_equal(r["vias"][0], m_in)
        if hb_in:
            np.testing.assert_array_equal(r["vias"][1], lb_in)
        smp = O.sample_tsp(m_in, s_in, lo, hi, 0.0, SEED + g, 0, samples)
        assert np.abs(r["vias"][nfx:] - smp).max() <= 1e-12
        if which == "flat_z":
            assert (r["vias"][nfx:, 0, 2] == 0.35).all()
        L, Cnf, Cwf, st, cost = O.tsp_score(stk["osc"], starts[g], ends[g], r["vias"], checks)
        np.testing.assert_array_equal(r["status"], st)
        fin = np.isfinite(cost)
        np.testing.assert_array_equal(np.isfinite(r["cost"]), fin)
        for a, b in ((r["cost"][fin], cost[fin]), (r["L"], L), (r["C_nf"], Cnf), (r["C_wf"], Cwf)):
            assert close(a, b, 1e-12)
        m, s, lb, hb, ns, el, bs = O.ces_update(r["cost"], r["status"], r["vias"], m_in, s_in, lb_in, hb_in,
                                                lo=lo, hi=hi)
        assert r["n_success"] == ns and r["best_slot"] == bs and r["has_best"] == hb
        np.testing.assert_array_equal(r["elites"], el)
        np.testing.assert_array_equal(bits(r["mean"]), bits(m))
        np.testing.assert_array_equal(bits(r["sigma"]), bits(s))
        np.testing.assert_array_equal(bits(r["last_best"]), bits(lb))
        succ += ns > 0
    assert succ >= 1
