"""Case generators for tests/test_ces_edges.py — TEST INFRASTRUCTURE ONLY.

Crafted candidate lists for the CES update (ces.hip: k_ces_rank / k_ces_scatter / k_ces_update),
distributions and bounds for the TaskSpacePlanner sampler (k_tsp's prologue) and via sets for the
many-via evaluation, plus an extended-precision restatement of the spline interpolation and arc
length that sets the many-via tolerance.  Everything here is plain numpy: no device, no oracle.
"""
import math

import numpy as np

LO, HI = (-0.5, -0.5, 0.0, -1.6), (0.5, 0.5, 0.6, 1.6)
PI_LO, PI_HI = (-0.5, -0.5, 0.0, -math.pi), (0.5, 0.5, 0.6, math.pi)
# O.ces_update's configuration names; CesPlanner's defaults
BASE = dict(frac=0.3, inc=1.5, dec=0.95, sigma_floor=0.0, var_beta=0.2, mean_lr=0.5, sd_min=0.01,
            sd_max=0.5, dist_z_min=0.3, lo=LO, hi=HI)
START, END = (0.205, 0.0, 0.12, 0.0), (0.0, 0.0, 0.32, 0.0)


def planner_kwargs(case):
    """CesPlanner keyword arguments of an update case (n slots = sample_count + 2)."""
    c = case["cfg"]
    return dict(sample_count=case["n"] - 2, check_points=8, init_points=case["K"] + 2,
                elite_fraction=c["frac"], stddev_increase_factor=c["inc"], stddev_decay_factor=c["dec"],
                sigma_floor=c["sigma_floor"], var_ema_beta=c["var_beta"], mean_lr=c["mean_lr"],
                stddev_min=c["sd_min"], stddev_max=c["sd_max"], stddev_initial=c["dist_z_min"],
                limits_min=c["lo"], limits_max=c["hi"])


def status_pattern(rng, n, succ):
    """succ: "all", "none", "last" (one success, in the last slot), an int (that many successes at
    random slots) or a float (success probability)."""
    st = np.zeros(n, np.uint8)
    if succ == "all":
        st[:] = 1
    elif succ == "last":
        st[-1] = 1
    elif succ == "none":
        pass
    elif isinstance(succ, (int, np.integer)):
        st[rng.choice(n, int(succ), replace=False)] = 1
    else:
        st[rng.uniform(size=n) < succ] = 1
    return st


def make_list(seed, n, K, succ=0.6, lo=LO, hi=HI, cost="ties", spread=0.2):
    """One iteration's candidate list: per-slot L, C_nf, C_wf, cost, status, vias [n][K][4].
    Via coordinates are uniform over the bounds widened by `spread` of the range on each side;
    cost "ties": uniform(0, 3) rounded to one decimal, "signed": uniform(-3, 3) rounded to one
    decimal, "cont": continuous."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    w = hi - lo
    vias = rng.uniform(lo - spread * w, hi + spread * w, (n, K, 4))
    st = status_pattern(rng, n, succ)
    if cost == "ties":
        c = np.round(rng.uniform(0.0, 3.0, n), 1)
    elif cost == "signed":
        c = np.round(rng.uniform(-3.0, 3.0, n), 1)
    else:
        c = rng.uniform(0.0, 3.0, n)
    L = rng.uniform(0.5, 2.0, n)
    Cnf = np.where(st, 0.0, rng.uniform(0.1, 1.0, n))
    Cwf = Cnf + rng.uniform(0.0, 0.5, n)
    return dict(L=L, C_nf=Cnf, C_wf=Cwf, cost=c, status=st, vias=vias)


def tie_runs(lst, value=0.1):
    """Runs of equal low cost across the 256-slot tile borders (slots 253..258 and 509..514),
    all successes: inside the elite set, so their order decides elites[] and the weights."""
    n = len(lst["cost"])
    for a in (253, 509):
        b = min(a + 6, n)
        if a < n:
            lst["cost"][a:b] = value
            lst["status"][a:b] = 1
            lst["C_nf"][a:b] = 0.0
    return lst


def pack(lst, n_slots, K):
    """The packed f64 records [L, C_nf, C_wf, cost, status, vias] sspp_ces_unpack reads, padded
    to n_slots with what an evaluation leaves in padding slots: status 0, cost +inf."""
    n = len(lst["cost"])
    rec = np.zeros((n_slots, 5 + 4 * K))
    rec[n:, :4] = np.inf
    rec[:n, 0], rec[:n, 1], rec[:n, 2], rec[:n, 3] = lst["L"], lst["C_nf"], lst["C_wf"], lst["cost"]
    rec[:n, 4] = lst["status"]
    rec[:n, 5:] = lst["vias"].reshape(n, 4 * K)
    return rec


def _state(seed, K, cfg, sigma=None):
    rng = np.random.default_rng(seed + 7919)
    lo, hi = np.asarray(cfg["lo"], float), np.asarray(cfg["hi"], float)
    mean = rng.uniform(lo, hi, (K, 4))
    mean[:, 2] = np.maximum(mean[:, 2], min(cfg["dist_z_min"], hi[2]))
    sg = rng.uniform(cfg["sd_min"], cfg["sd_max"], (K, 4)) if sigma is None else np.broadcast_to(
        np.asarray(sigma, float), (K, 4)).copy()
    lbest = rng.uniform(lo, hi, (K, 4))
    return mean, sg, lbest


def case(id, n, K=1, lists=None, mean=None, sigma=None, lbest=None, world=1, seed=0, succ=0.6,
         cost="ties", **cfg):
    c = dict(BASE, **cfg)
    if lists is None:
        lists = [make_list(seed, n, K, succ, c["lo"], c["hi"], cost)]
    m, s, lb = _state(seed, K, c, sigma)
    return dict(id=id, n=n, K=K, cfg=c, lists=lists, world=world,
                mean=m if mean is None else np.asarray(mean, float).reshape(K, 4),
                sigma=s, lbest=lb if lbest is None else np.asarray(lbest, float).reshape(K, 4))


def _with_successes(seed, n, K, nsucc):
    return [make_list(seed, n, K, int(nsucc))]


def update_cases():
    """Every crafted update case, {id: case}.  n is the planner's list size (sample_count + 2)."""
    out = []
    # list sizes around the fused / three-launch switch (512) and the 256-slot rank tiles
    for i, n in enumerate((3, 64, 65, 256, 257, 512, 513, 1025)):
        out.append(case("size%d" % n, n, lists=[tie_runs(make_list(10 + i, n, 1, 0.6))], seed=10 + i))
    # elite counts: k = 1, 2, 511, 512, 513 (s_idx / s_wt over one pass of 512 lanes), 1024 / 1025
    # (elites cached in registers or re-loaded), 8192 (both LDS arrays full)
    out.append(case("k1", 3, succ="last", seed=20))
    out.append(case("k2", 9, lists=_with_successes(21, 9, 1, 7), seed=21))
    out.append(case("k511", 513, lists=_with_successes(22, 513, 1, 511), frac=1.0, seed=22))
    out.append(case("k512", 512, succ="all", frac=1.0, seed=23))
    out.append(case("k513", 513, succ="all", frac=1.0, seed=24))
    out.append(case("k1024", 1025, lists=_with_successes(25, 1025, 1, 1024), frac=1.0, seed=25))
    out.append(case("k1025", 1025, succ="all", frac=1.0, seed=26))
    out.append(case("k8192", 8192, succ="all", frac=1.0, seed=27))
    # ties: every cost equal (the elites must be the lowest slots, across tiles), +-0 mixed,
    # negative costs, a +inf success among finite ones
    for n in (300, 513):
        lst = make_list(30 + n, n, 1, "all")
        lst["cost"][:] = 1.25
        out.append(case("equal%d" % n, n, lists=[lst], seed=30))
    for n in (64, 300):
        lst = make_list(31 + n, n, 1, 0.8)
        lst["cost"] = np.where(np.arange(n) % 3 == 0, 0.0, -0.0)
        lst["cost"][n // 2] = 0.5
        out.append(case("zeros%d" % n, n, lists=[lst], frac=0.5, seed=31))
    for n in (64, 600):
        out.append(case("negative%d" % n, n, cost="signed", seed=32 + n))
    for n in (6, 300):
        lst = make_list(33 + n, n, 1, "all", cost="ties")
        lst["cost"][1] = np.inf
        lst["cost"][n - 2] = np.inf
        out.append(case("inf%d" % n, n, lists=[lst], frac=1.0, seed=33))
    # success patterns
    for n in (64, 600):
        out.append(case("none%d" % n, n, succ="none", seed=40))
        out.append(case("last%d" % n, n, succ="last", seed=41))
        out.append(case("all%d" % n, n, succ="all", seed=42))
    # elite-count rounding: int(nsucc * frac) at products one ulp from an integer
    for i, (ns, fr) in enumerate(((100, 0.29), (100, 0.57), (100, 0.07), (10, 0.3), (7, 0.3), (3, 0.0))):
        for n in (160, 600):
            out.append(case("round_%d_%s_n%d" % (ns, fr, n), n, lists=_with_successes(50 + i, n, 1, ns),
                            frac=fr, seed=50 + i))
    # yaw: elites on both sides of the +-pi seam; a range far narrower than the spread (about 16
    # wrap turns; everything finite and within 40 ranges of the bounds); lo[3] == hi[3]
    lst = make_list(60, 6, 1, "all")
    lst["status"][4:] = 0
    lst["vias"][:4, 0, 3] = [3.1, -3.1, 3.05, -3.05]
    lst["cost"][:4] = [1.0, 1.1, 1.2, 1.3]
    # (stddev_max = 4 keeps the yaw sigma off its clamp, so the wrapped variance shows; with
    # mean_lr = 0 the mean stays on the seam and the default stddev_max does)
    out.append(case("seam6", 6, lists=[lst], lo=PI_LO, hi=PI_HI, frac=1.0, mean=[0.0, 0.0, 0.5, 3.1], sd_max=4.0))
    out.append(case("seam6_keep", 6, lists=[lst], lo=PI_LO, hi=PI_HI, frac=1.0, mean=[0.0, 0.0, 0.5, 3.1],
                    mean_lr=0.0, sigma=0.1))
    for n in (64, 700):
        lst = make_list(61 + n, n, 2, 0.7, PI_LO, PI_HI)
        r = np.random.default_rng(61)
        lst["vias"][:, :, 3] = np.where(r.uniform(size=(n, 2)) < 0.5, 1.0, -1.0) * r.uniform(2.9, math.pi, (n, 2))
        out.append(case("seam%d" % n, n, K=2, lists=[lst], lo=PI_LO, hi=PI_HI, seed=61, sd_max=4.0,
                        mean=[0.0, 0.0, 0.5, 3.1, 0.1, 0.1, 0.4, -3.0]))
    nlo, nhi = (-0.5, -0.5, 0.0, -0.1), (0.5, 0.5, 0.6, 0.1)
    for n in (64, 700):
        lst = make_list(62 + n, n, 1, 0.7, nlo, nhi)
        lst["vias"][:, 0, 3] = np.random.default_rng(62).uniform(-3.1, 3.1, n)
        out.append(case("narrowyaw%d" % n, n, lists=[lst], lo=nlo, hi=nhi, seed=62))
    flo, fhi = (-0.5, -0.5, 0.0, 0.25), (0.5, 0.5, 0.6, 0.25)
    for n in (64, 700):
        lst = make_list(63 + n, n, 1, 0.7, flo, fhi)
        lst["vias"][:, 0, 3] = np.random.default_rng(63).uniform(-3.0, 3.0, n)
        out.append(case("fixedyaw%d" % n, n, lists=[lst], lo=flo, hi=fhi, seed=63))
    # mean clamps: the weighted elite mean lands above hi (x), below lo (y) and below dist_z_min (z)
    for n in (64, 600):
        lst = make_list(64 + n, n, 2, 0.7)
        lst["vias"][:, :, 0] += 1.5
        lst["vias"][:, :, 1] -= 1.5
        lst["vias"][:, :, 2] = np.random.default_rng(64).uniform(0.0, 0.2, (n, 2))
        out.append(case("meanclamp%d" % n, n, K=2, lists=[lst], mean_lr=1.0, seed=64))
    # sigma clamps: incoming sigma at stddev_min, at stddev_max, at 0; sigma_floor > stddev_max
    srow = [0.01, 0.5, 0.0, 0.2]
    for n in (64, 600):
        out.append(case("sigmaedges%d" % n, n, sigma=srow, seed=65))
        out.append(case("sigmaedges_none%d" % n, n, sigma=srow, succ="none", seed=65))
        out.append(case("floor%d" % n, n, sigma=srow, sigma_floor=0.7, seed=66))
        out.append(case("floor_none%d" % n, n, sigma=srow, sigma_floor=0.7, succ="none", seed=66))
    for vb in (0.0, 1.0):
        for lr in (0.0, 1.0):
            for n in (64, 600):
                out.append(case("beta%g_lr%g_n%d" % (vb, lr, n), n, var_beta=vb, mean_lr=lr, seed=67))
    # via counts (K = 1 throughout above)
    for K in (3, 32):
        for n in (64, 513):
            out.append(case("vias%d_n%d" % (K, n), n, K=K, seed=70 + K))
    return {c["id"]: c for c in out}


def rearm_case():
    """Four updates on one planner: all 600 slots succeed, then 17, then none, then all again —
    rank[] and the success counter must be re-armed by each update for the next."""
    n = 600
    a = make_list(80, n, 1, "all")
    return case("rearm", n, lists=[a, make_list(81, n, 1, 17), make_list(82, n, 1, "none"), a], frac=1.0,
                seed=80)


def padding_case():
    """101 live slots: world 2 and 3 both round the list up to 102 slots, one of padding."""
    return case("padding", 101, K=2, seed=83)


def special_list(n=300, K=2):
    """-0.0, +inf and subnormals in every field (pack / unpack round trip)."""
    lst = make_list(84, n, K, 0.5, cost="cont")
    tiny = np.float64(5e-324)
    for k, f in enumerate(("L", "C_nf", "C_wf", "cost")):
        lst[f][k::16] = -0.0
        lst[f][k + 4::16] = np.inf
        lst[f][k + 8::16] = tiny * (k + 1)
        lst[f][k + 12::16] = -2.2250738585072014e-308 / 4
    v = lst["vias"].reshape(-1)
    v[0::7] = -0.0
    v[3::11] = tiny
    v[5::13] = np.inf
    return lst


# ------------------------------------------------------------------ sampler cases
def sampler_cases():
    """{id: dict(K, mean, sigma, lo, hi, z_min)} for 4096 samples each."""
    out = {}

    def add(id, mean, sigma, lo=LO, hi=HI, z_min=0.0):
        mean = np.asarray(mean, float).reshape(-1, 4)
        out[id] = dict(K=mean.shape[0], mean=mean,
                       sigma=np.broadcast_to(np.asarray(sigma, float), mean.shape).copy(),
                       lo=tuple(lo), hi=tuple(hi), z_min=float(z_min))
    m = [0.1, -0.1, 0.3, 0.2]
    for i in range(3):  # lo[i] == hi[i]: every sample of that coordinate takes the fallback
        lo, hi = list(LO), list(HI)
        lo[i] = hi[i] = (0.05, -0.05, 0.35)[i]
        add("degenerate%d" % i, m, 0.3, lo, hi)
    # a window of 0.0175 sigma around the mean: acceptance 0.399 * 0.0175 = 0.7 % per draw, so
    # 1 - (1 - 0.007)^99 = 50 % of the samples are accepted within 99 draws, the rest fall back
    for i in range(3):
        lo, hi = list(LO), list(HI)
        lo[i], hi[i] = m[i] - 0.5 * 0.0175 * 0.3, m[i] + 0.5 * 0.0175 * 0.3
        add("narrow%d" % i, m, 0.3, lo, hi)
    for i in range(3):  # mean exactly on hi[i], sigma = stddev_max
        mm = list(m)
        mm[i] = HI[i]
        add("meanonbound%d" % i, mm, 0.5)
    add("yaw_mean_on_hi", [0.1, -0.1, 0.3, HI[3]], [0.3, 0.3, 0.3, 0.5])
    add("yaw_many_wraps", m[:3] + [0.01], [0.3, 0.3, 0.3, 0.5], LO[:3] + (-0.05,), HI[:3] + (0.05,))
    add("yaw_fixed", m, 0.3, LO[:3] + (0.25,), HI[:3] + (0.25,))
    add("zclamp", m, 0.3, z_min=0.25)  # lo[2] = 0 < z_min < hi[2] = 0.6
    r = np.random.default_rng(90)       # every via its own mean and sigma: Philox index of each
    mean32 = r.uniform(np.asarray(LO) * 0.8, np.asarray(HI) * 0.8, (32, 4))
    mean32[:, 2] = r.uniform(0.1, 0.5, 32)
    add("vias32", mean32, r.uniform(0.02, 0.5, (32, 4)))
    return out


# ------------------------------------------------------------------ many-via evaluation
def via_sets(K, B, start, end, seed, sigma_free=0.004, sigma_hit=0.05, dip=0.0):
    """B via sets around the straight line start -> end: the first half with a small spread
    (sigma_free), the second half with sigma_hit and its middle vias lowered by `dip`."""
    rng = np.random.default_rng(seed)
    start, end = np.asarray(start, float), np.asarray(end, float)
    t = (np.arange(1, K + 1) / (K + 1))[:, None]
    line = (1.0 - t) * start + t * end
    v = np.repeat(line[None], B, 0)
    h = B // 2
    v[:h] += sigma_free * rng.standard_normal((h, K, 4))
    v[h:] += sigma_hit * rng.standard_normal((B - h, K, 4))
    mid = slice(K // 3, max(K // 3 + 1, 2 * K // 3))
    v[h:, mid, 2] -= dip
    return v


def _ld(x):
    return np.asarray(x, dtype=np.longdouble)


def _basis_ld(u, knots, n):
    """Span and the three degree-2 basis values at u (Piegl & Tiller A2.1 / A2.2), longdouble."""
    p = 2
    if u >= knots[n]:
        span = n - 1
    else:
        span = int(np.searchsorted(knots, u, side="right")) - 1
        span = min(max(span, p), n - 1)
    N = [np.longdouble(1)] + [np.longdouble(0)] * p
    left, right = [np.longdouble(0)] * (p + 1), [np.longdouble(0)] * (p + 1)
    for j in range(1, p + 1):
        left[j] = u - knots[span + 1 - j]
        right[j] = knots[span + j] - u
        saved = np.longdouble(0)
        for r in range(j):
            tmp = N[r] / (right[r + 1] + left[j - r])
            N[r] = saved + right[r + 1] * tmp
            saved = left[j - r] * tmp
        N[j] = saved
    return span, N


def arc_length_longdouble(start, end, vias, cp):
    """PathModel::fromVias + the arc length of Evaluator::eval_one_pass restated in np.longdouble:
    the degree-2 B-spline through [start, vias..., end] at u_i = i / (n - 1) with averaged knots
    (collocation system solved by Gaussian elimination with partial pivoting), then the sum of the
    cp chords between s(i / cp).  vias [B][K][4] -> L [B] (longdouble)."""
    vias = _ld(vias)
    B, K, _ = vias.shape
    n, p = K + 2, 2
    one = np.longdouble(1)
    u = _ld(np.arange(n)) / np.longdouble(n - 1)
    knots = np.zeros(n + p + 1, np.longdouble)
    knots[n:] = one
    for j in range(1, n - p):
        knots[j + p] = (u[j] + u[j + 1]) / np.longdouble(2)
    A = np.zeros((n, n), np.longdouble)
    A[0, 0] = A[n - 1, n - 1] = one
    for i in range(1, n - 1):
        span, N = _basis_ld(u[i], knots, n)
        for r in range(p + 1):
            A[i, span - p + r] = N[r]
    pts = np.concatenate([np.broadcast_to(_ld(start), (B, 1, 4)), vias,
                          np.broadcast_to(_ld(end), (B, 1, 4))], axis=1)
    X = np.ascontiguousarray(pts.transpose(1, 0, 2).reshape(n, B * 4))
    for k in range(n):  # elimination, partial pivoting
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            X[[k, piv]] = X[[piv, k]]
        for i in range(k + 1, min(n, k + 4)):  # the matrix is banded: 3 entries per row
            if A[i, k] != 0:
                f = A[i, k] / A[k, k]
                A[i, k:] -= f * A[k, k:]
                X[i] -= f * X[k]
    for i in range(n - 1, -1, -1):
        X[i] = (X[i] - A[i, i + 1:] @ X[i + 1:]) / A[i, i]
    ctrl = X.reshape(n, B, 4)
    L = np.zeros(B, np.longdouble)
    prev = None
    for i in range(cp + 1):
        span, N = _basis_ld(np.longdouble(i) / np.longdouble(cp), knots, n)
        cur = N[0] * ctrl[span - 2] + N[1] * ctrl[span - 1] + N[2] * ctrl[span]
        if prev is not None:
            L += np.sqrt(((cur - prev) ** 2).sum(axis=1))
        prev = cur
    return L
