"""Independent numpy reference for cylinder-cylinder pairs (the CPU oracle has none).

Cylinder i: centre c_i, unit axis a_i, radius R_i, half height H_i; support function
h_i(n) = H_i |a_i.n| + R_i sqrt(1 - (a_i.n)^2).  The signed distance is

    sd = max over unit n of  n.(c_2 - c_1) - h_1(n) - h_2(n)

(the distance of separated bodies, minus the penetration depth of overlapping ones).  `sd`
maximises that by brute force — a dense Fibonacci sphere, then an adaptive random search around
the best samples — with no reasoning about candidate axes, vectorised over pairs.

Accuracy, measured by tests/test_cylcyl_ref.py::test_reference_accuracy on the configurations
with an analytic signed distance (`analytic_families`): the maximum error E found is 3.1e-10 (the
rim-rim diagonal within 1e-9 of touching, where the radial and the axial direction are two maxima
2e-10 apart and the search can settle on the lower; every other family is below 1e-10, most
below 1e-13).  E_MAX = 5e-10 is asserted there, so the "near" band |sd - thr| <= BAND inside which
no decision is compared is 10 E_MAX = 5e-9 (the floor would be the project's 1e-9).

The rule (MuJoCo's convex collider as for cylinder-box): one contact iff
sd < margin, deep iff sd < -1e-3.
"""
import math

import numpy as np

DEEP = -1e-3
E_MAX = 5e-10     # asserted bound of the reference's error on the analytic cases
BAND = 5e-9       # max(10 E_MAX, 1e-9)


def fib_sphere(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = math.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)


def _perp(n, a):
    """|a x n| for n (..., 3) against a (..., 3): sqrt(1 - (a.n)^2) without the cancellation"""
    c = np.cross(np.broadcast_to(a, n.shape), n)
    return np.sqrt((c * c).sum(-1))


def sep(n, T, a1, R1, H1, a2, R2, H2):
    """separation along the unit directions n (N, M, 3) of N pairs (T, a1, a2: (N, 3))"""
    T, a1, a2 = T[:, None, :], a1[:, None, :], a2[:, None, :]
    h1 = H1[:, None] * np.abs((n * a1).sum(-1)) + R1[:, None] * _perp(n, a1)
    h2 = H2[:, None] * np.abs((n * a2).sum(-1)) + R2[:, None] * _perp(n, a2)
    return np.abs((n * T).sum(-1)) - h1 - h2


_DENSE = {}


def sd(T, a1, R1, H1, a2, R2, H2, dense=12000, starts=12, cands=48, rounds=300, seed=0, chunk=256):
    """signed distance of N pairs; every argument has leading dimension N (scalars broadcast).
    The starts are the best dense sample of each of `starts` regions of the sphere (a penetrating
    pair has several local maxima, and the best few samples all sit on one).  The search around each adapts its own step (longer after a gain,
    shorter after none) and draws each step's length over several decades, so it follows the
    narrow ridges a rim leaves in the objective; a quarter of the steps repeat the last gaining step
    at other lengths, a quarter each are projected onto a cylinder's crease a.n = 0 (a random step
    never lands on one), a quarter stay as drawn."""
    T = np.atleast_2d(np.asarray(T, float))
    N = len(T)
    a1 = np.broadcast_to(np.asarray(a1, float), (N, 3))
    a2 = np.broadcast_to(np.asarray(a2, float), (N, 3))
    R1, H1, R2, H2 = (np.broadcast_to(np.asarray(x, float), (N,)) for x in (R1, H1, R2, H2))
    if (dense, starts) not in _DENSE:
        pts = fib_sphere(dense)
        _DENSE[(dense, starts)] = (pts, (pts @ fib_sphere(starts).T).argmax(1))
    ns, region = _DENSE[(dense, starts)]
    rng = np.random.default_rng(seed)
    out = np.empty(N)
    for lo in range(0, N, chunk):
        s = slice(lo, min(N, lo + chunk))
        args = (T[s], a1[s], R1[s], H1[s], a2[s], R2[s], H2[s])
        m = s.stop - s.start
        v = sep(np.broadcast_to(ns, (m, dense, 3)), *args)
        top = np.stack([np.flatnonzero(region == r)[v[:, region == r].argmax(1)] for r in range(starts)], 1)
        bn = ns[top]                                   # (m, starts, 3)
        bv = np.take_along_axis(v, top, 1)
        scale = np.full((m, starts), 0.03)
        mv = np.zeros((m, starts, 3))                  # the last gaining step
        for _ in range(rounds):
            step = scale[:, :, None, None] * 10.0 ** rng.uniform(-2.0, 0.3, size=(m, starts, cands, 1))
            c = bn[:, :, None, :] + step * rng.normal(size=(m, starts, cands, 3))
            for a, k0 in ((args[1], 0), (args[4], 1)):
                sub = c[:, :, k0::4, :]
                sub -= (sub * a[:, None, None, :]).sum(-1, keepdims=True) * a[:, None, None, :]
            # ... and a quarter repeat the last gaining step, longer, shorter and reversed
            c[:, :, 2::4, :] = bn[:, :, None, :] + mv[:, :, None, :] * (
                rng.choice([-1.0, 1.0], size=(m, starts, 1, 1)) * 10.0 ** rng.uniform(-1.5, 1.5, size=(m, starts, len(range(2, cands, 4)), 1)))
            c /= np.maximum(np.linalg.norm(c, axis=-1, keepdims=True), 1e-300)
            cv = sep(c.reshape(m, -1, 3), *args).reshape(m, starts, cands)
            k = cv.argmax(2)
            kv = np.take_along_axis(cv, k[:, :, None], 2)[:, :, 0]
            better = kv > bv
            kn = np.take_along_axis(c, k[:, :, None, None], 2)[:, :, 0, :]
            mv = np.where(better[:, :, None], kn - bn, mv)
            bn = np.where(better[:, :, None], kn, bn)
            bv = np.where(better, kv, bv)
            scale = np.clip(np.where(better, scale * 1.25, scale * 0.86), 1e-13, 0.3)
        out[s] = bv.max(1)
    return out


def decide(dist, margin):
    """(contacts, deep) of the rule from signed distances"""
    c = dist < margin
    return c.astype(int), (c & (dist < DEEP)).astype(int)


def vertical_sd(T, R1, H1, R2, H2):
    dr = np.hypot(T[..., 0], T[..., 1]) - (R1 + R2)
    dz = np.abs(T[..., 2]) - (H1 + H2)
    both = (dr > 0) & (dz > 0)
    return np.where(both, np.hypot(dr, dz), np.maximum(dr, dz))


def cheap3(T, a1, R1, H1, a2, R2, H2):
    """the lower bound of the three axes a_1, a_2, a_1 x a_2 alone"""
    T = np.atleast_2d(T)
    N = len(T)
    a1 = np.broadcast_to(a1, (N, 3))
    a2 = np.broadcast_to(a2, (N, 3))
    x = np.cross(a1, a2)
    ln = np.linalg.norm(x, axis=1, keepdims=True)
    x = np.where(ln > 1e-6, x / np.maximum(ln, 1e-300), a1)
    n = np.stack([a1, a2, x], 1)
    b = lambda v: np.broadcast_to(np.asarray(v, float), (N,))  # noqa: E731
    return sep(n, T, a1, b(R1), b(H1), a2, b(R2), b(H2)).max(1)


def rot_axis(axis, ang):
    """rotation matrix about a unit axis (Rodrigues)"""
    axis = np.asarray(axis, float)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


# ---------------------------------------------------------------- analytic configurations
# Each family: (name, M1, (R1, H1), M2, (R2, H2), direction d, touching offset t0) — cylinder 1
# at the origin with rotation M1, cylinder 2 with rotation M2 at T = d * (t0 + gap): the signed
# distance is exactly `gap` for |gap| small against the sizes (the closest feature pair and its
# normal d do not change).
def analytic_families():
    R1, H1, R2, H2 = 0.05, 0.08, 0.03, 0.06
    I = np.eye(3)
    fam = []
    ex, ey, ez = np.eye(3)
    # parallel, side by side
    fam.append(("parallel_side", I, (R1, H1), I, (R2, H2), ex, R1 + R2, np.zeros(3)))
    # stacked cap to cap (slightly off axis)
    fam.append(("stacked_caps", I, (R1, H1), I, (R2, H2), ez, H1 + H2, np.array([0.01, 0.02, 0.0])))
    # rim-rim diagonal of the parallel case: the offset (dr, dz) past both the radii and the heights
    dg = np.array([math.cos(0.7), 0.0, math.sin(0.7)])
    fam.append(("rim_rim_diagonal", I, (R1, H1), I, (R2, H2), dg, 0.0,
                np.array([R1 + R2, 0.0, H1 + H2])))
    # perpendicular crossed axes: sd = axis distance - R1 - R2
    Mx = rot_axis(ey, math.pi / 2)  # axis of 2 along x
    fam.append(("crossed", rot_axis(ex, math.pi / 2), (R1, H1), Mx, (R2, H2), ez, R1 + R2, np.zeros(3)))
    # cylinder 2 lying across cylinder 1's cap: sd = dz - H1 - R2
    fam.append(("lying_on_cap", I, (R1, H1), Mx, (R2, H2), ez, H1 + R2, np.array([0.01, 0.0, 0.0])))
    # tilted cylinder 2 over the cap of 1: sd = dz - H1 - h2(a1), low point over the disc
    Mt = rot_axis(ey, 0.4)
    h2 = H2 * abs(Mt[2, 2]) + R2 * math.sqrt(1 - Mt[2, 2] ** 2)
    fam.append(("tilted_on_cap", I, (R1, H1), Mt, (R2, H2), ez, H1 + h2, np.zeros(3)))
    # rim against rim, skew axes (separated only: POSITIVE_ONLY): the rim point p of cylinder 1, a
    # normal n inside p's normal cone, cylinder 2 placed so that its rim point q = p + gap n has -n
    # inside q's normal cone; n separates, so the distance is the gap
    p = np.array([R1, 0.0, H1])
    n = np.array([math.cos(0.6), 0.0, math.sin(0.6)])
    e = np.cross(-n, np.array([0.3, 1.0, 0.2]))
    e /= np.linalg.norm(e)
    rho, k = math.cos(0.5) * -n - math.sin(0.5) * e, math.sin(0.5) * -n + math.cos(0.5) * e
    fam.append(("rim_rim_skew", I, (R1, H1), np.stack([rho, np.cross(k, rho), k], 1), (R2, H2), n, 0.0,
                p - R2 * rho - H2 * k))
    return fam


POSITIVE_ONLY = ("rim_rim_skew",)


def family_pose(f, gap):
    """(T, a1, R1, H1, a2, R2, H2, M1, M2) of an analytic family at signed distance `gap`"""
    name, M1, (R1, H1), M2, (R2, H2), d, t0, base = f
    T = base + d * (t0 + gap)
    return T, M1[:, 2], R1, H1, M2[:, 2], R2, H2, M1, M2


def sd_for_gap(f, want):
    """the gap that gives family f the signed distance `want` (the rim-rim diagonal's depth
    below touching is max(d_r, d_z), not the offset along the diagonal)"""
    if f[0] == "rim_rim_diagonal" and want < 0:
        return want / min(abs(f[5][0]), abs(f[5][2]))
    return want


# ---------------------------------------------------------------- whole scenes
def _depth_in(p, c, a, R, H):
    """depth of the points p (N, K, 3) inside the cylinders (c, a, R, H: per N); <= 0 outside"""
    w = p - c[:, None, :]
    z = (w * a[:, None, :]).sum(-1)
    rho = np.sqrt(np.maximum((w * w).sum(-1) - z * z, 0.0))
    return np.minimum(R[:, None] - rho, H[:, None] - np.abs(z))


def _body_points(c, a, R, H):
    """points of the cylinders (c, a, R, H: per N): (N, K, 3) — the axis segment, and rings at
    half and full radius at five heights"""
    N = len(c)
    e = np.where(np.abs(a[:, :1]) < 0.7, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    u = np.cross(a, e)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(a, u)
    ts = np.linspace(-1.0, 1.0, 5)
    ang = np.arange(8) * (math.pi / 4)
    pts = [c[:, None, :] + t * H[:, None, None] * a[:, None, :] for t in np.linspace(-1.0, 1.0, 9)]
    for t in ts:
        for f in (0.5, 1.0):
            ring = np.cos(ang)[None, :, None] * u[:, None, :] + np.sin(ang)[None, :, None] * v[:, None, :]
            pts.append(c[:, None, :] + t * H[:, None, None] * a[:, None, :] + f * R[:, None, None] * ring)
    return np.concatenate([x if x.ndim == 3 else x[:, None, :] for x in pts], 1)


SCENE_SD = dict(dense=4000)  # scene_sd's search (checked against sd's)


def scene_bounds(T, a1, R1, H1, a2, R2, H2, thr, slack=1e-6):
    """The cheap half of scene_sd: (distances — a bound where one decides, else nan; undecided)."""
    N = len(T)
    R1, H1, R2, H2 = (np.broadcast_to(np.asarray(x, float), (N,)) for x in (R1, H1, R2, H2))
    out = np.full(N, np.nan)
    todo = np.ones(N, bool)

    def directions(ndir):
        idx = np.flatnonzero(todo)
        ns = fib_sphere(ndir)
        for lo in range(0, len(idx), 2048):
            i = idx[lo:lo + 2048]
            lb = sep(np.broadcast_to(ns, (len(i), ndir, 3)), T[i], a1[i], R1[i], H1[i], a2[i], R2[i], H2[i]).max(1)
            far = lb > thr + slack
            out[i[far]] = lb[far]
            todo[i[far]] = False

    # bounding spheres, then a coarse sphere of directions
    lb = np.sqrt((T * T).sum(1)) - np.hypot(R1, H1) - np.hypot(R2, H2)
    out[lb > thr + slack] = lb[lb > thr + slack]
    todo &= ~(lb > thr + slack)
    directions(300)
    idx = np.flatnonzero(todo)
    for lo in range(0, len(idx), 2048):
        i = idx[lo:lo + 2048]
        o = np.zeros((len(i), 3))
        dep = np.maximum(_depth_in(_body_points(T[i], a2[i], R2[i], H2[i]), o, a1[i], R1[i], H1[i]).max(1),
                         _depth_in(_body_points(o, a1[i], R1[i], H1[i]), T[i], a2[i], R2[i], H2[i]).max(1))
        deep = dep > slack - min(thr, 0.0)
        out[i[deep]] = -dep[deep]
        todo[i[deep]] = False
    directions(5000)
    return out, todo


def scene_search(out, idx, T, a1, R1, H1, a2, R2, H2, **kw):
    """fill out[idx] with the searched distances (SCENE_SD's search)"""
    N = len(T)
    R1, H1, R2, H2 = (np.broadcast_to(np.asarray(x, float), (N,)) for x in (R1, H1, R2, H2))
    if len(idx):
        out[idx] = sd(T[idx], a1[idx], R1[idx], H1[idx], a2[idx], R2[idx], H2[idx], **dict(SCENE_SD, **kw))
    return out


def scene_sd(T, a1, R1, H1, a2, R2, H2, thr, slack=1e-6, **kw):
    """Signed distances of many pairs where the decision sd < thr (thr = the margin, or DEEP) needs
    them.  A pair that its bounding spheres or some direction of a coarse sphere separate by more
    than thr + slack gets that lower bound; a pair with a point of one cylinder deeper than
    slack - min(thr, 0) inside the other gets minus that depth (an upper bound: a ball around a
    point of one body inside the other); the rest get `sd`.  Either bound is farther than `slack`
    from thr, on the side the exact value is on, so the decision and the near band taken from the
    result are those of `sd`.  Returns (distances, which were searched)."""
    out, todo = scene_bounds(T, a1, R1, H1, a2, R2, H2, thr, slack)
    return scene_search(out, np.flatnonzero(todo), T, a1, R1, H1, a2, R2, H2, **kw), todo
