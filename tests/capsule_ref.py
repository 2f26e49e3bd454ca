"""numpy reference for the capsule colliders — TEST INFRASTRUCTURE ONLY.

The CPU oracle (oracle/) knows no capsule, so the capsule contact rules of DESIGN.md §4 are
restated here, literally, per pair type.  Everything is vectorised over a leading axis of N
pairs: positions [N, 3], rotations [N, 9] (row-major, columns = the frame's axes), sizes [N, 3],
margin [N] (anything broadcastable).  Each rule returns (contacts [N], deep [N], dists [N, k]):
`dists` holds the signed distance of every sphere test the rule ran, in its order (nan: not
run); contact iff dist <= margin, deep iff it is a contact and dist < -1e-3.  A capsule is the
segment pos +- size[1] * (z column) with radius size[0].

The second half holds an INDEPENDENT distance per pair type (another algorithm), used only to
validate the rules above (tests/test_capsule_ref.py).
"""
import numpy as np

DEEP = -1e-3
MINVAL = 1e-15
PLANE, SPHERE, CAPSULE, CYLINDER, BOX = 0, 2, 3, 5, 6


def _a(x, last):
    x = np.asarray(x, float)
    return x.reshape((-1, last)) if x.ndim <= 1 else x


def dot(a, b):
    return (a * b).sum(-1)


def zcol(m):
    return _a(m, 9)[:, [2, 5, 8]]


def to_frame(m, v):
    """The frame's coordinates of v: (columns of m) . v."""
    m = _a(m, 9).reshape(-1, 3, 3)
    return np.einsum("nij,ni->nj", m, v)


def _tally(d, margin, run=None):
    """(contacts, deep, dists) of the tests d [N, k]; run: which of them were run."""
    margin = np.asarray(margin, float).reshape(-1, 1)
    c = d <= margin
    if run is not None:
        c &= run
        d = np.where(run, d, np.nan)
    return c.sum(1), (c & (d < DEEP)).sum(1), d


def _ss(p1, r1, p2, r2):
    return np.linalg.norm(p2 - p1, axis=-1) - (r1 + r2)


# ------------------------------------------------------------------ the rules
def plane_capsule(pp, pm, cp, cm, cs, margin):
    """One sphere-plane test per segment end, +h then -h."""
    pp, cp, cs = _a(pp, 3), _a(cp, 3), _a(cs, 3)
    n, a = zcol(pm), zcol(cm)
    r, h = cs[:, 0], cs[:, 1]
    d = np.stack([dot(n, cp + s[:, None] * a - pp) - r for s in (h, -h)], 1)
    return _tally(d, margin)


def sphere_capsule(sp, rs, cp, cm, cs, margin):
    """x = clamp(a . (s - c), -h, h); sphere-sphere against radius r at c + x a."""
    sp, cp, cs = _a(sp, 3), _a(cp, 3), _a(cs, 3)
    a = zcol(cm)
    x = np.clip(dot(a, sp - cp), -cs[:, 1], cs[:, 1])
    return _tally(_ss(sp, np.asarray(rs, float), cp + x[:, None] * a, cs[:, 0])[:, None], margin)


def capsule_capsule(p1, m1, s1, p2, m2, s2, margin):
    p1, p2, s1, s2 = _a(p1, 3), _a(p2, 3), _a(s1, 3), _a(s2, 3)
    a1, a2 = zcol(m1), zcol(m2)
    r1, h1, r2, h2 = s1[:, 0], s1[:, 1], s2[:, 0], s2[:, 1]
    dif = p1 - p2
    ma, mb, mc = dot(a1, a1), -dot(a1, a2), dot(a2, a2)
    u, v = -dot(a1, dif), dot(a2, dif)
    det = ma * mc - mb * mb
    par = np.abs(det) < MINVAL
    margin = np.broadcast_to(np.asarray(margin, float), par.shape)
    # general position: x1 from the 2x2 system, clamped; x2 for that x1 (the system's x2 when x1
    # is unclamped); x2 clamped and x1 recomputed, clamped; one sphere-sphere test
    with np.errstate(divide="ignore", invalid="ignore"):
        x1 = np.clip((mc * u - mb * v) / det, -h1, h1)
    x2 = (v - mb * x1) / mc
    hi, lo = x2 > h2, x2 < -h2
    x1 = np.where(hi, np.clip((u - mb * h2) / ma, -h1, h1), np.where(lo, np.clip((u + mb * h2) / ma, -h1, h1), x1))
    x2 = np.clip(x2, -h2, h2)
    dg = np.full((len(par), 4), np.nan)
    dg[:, 0] = _ss(p1 + x1[:, None] * a1, r1, p2 + x2[:, None] * a2, r2)
    run_g = np.zeros((len(par), 4), bool)
    run_g[:, 0] = True
    # parallel axes: end +h1, -h1 of capsule 1 against its nearest point of segment 2, then end
    # +h2, -h2 of capsule 2 against segment 1, until two contacts are found
    dp = np.empty((len(par), 4))
    for t, s in enumerate((h1, -h1)):
        e = p1 + s[:, None] * a1
        q = p2 + np.clip(dot(a2, e - p2), -h2, h2)[:, None] * a2
        dp[:, t] = _ss(e, r1, q, r2)
    for t, s in enumerate((h2, -h2)):
        e = p2 + s[:, None] * a2
        q = p1 + np.clip(dot(a1, e - p1), -h1, h1)[:, None] * a1
        dp[:, 2 + t] = _ss(q, r1, e, r2)
    cp = dp <= margin[:, None]
    before = np.concatenate([np.zeros((len(par), 1), int), np.cumsum(cp, 1)[:, :3]], 1)
    run_p = before < 2
    d = np.where(par[:, None], dp, dg)
    return _tally(d, margin, np.where(par[:, None], run_p, run_g))


def _dF(P, d, e, t):
    p = P + t[:, None] * d
    return dot(p - np.clip(p, -e, e), d)


def seg_box_dist(P, d, e, h):
    """Distance of the segments P + t d, |t| <= h, to the boxes |x_k| <= e_k (box frame): F' at
    the ends and at the breakpoints p_k = +-e_k clipped to [-h, h], the tightest bracket of its
    sign change, one linear interpolation."""
    lo, hi = -h, h.copy()
    glo, ghi = _dF(P, d, e, lo), _dF(P, d, e, hi)
    at_lo, at_hi = glo >= 0.0, (glo < 0.0) & (ghi <= 0.0)
    for k in range(3):
        for f in (-e[:, k], e[:, k]):
            with np.errstate(divide="ignore", invalid="ignore"):
                tb = np.where(d[:, k] != 0.0, np.clip((f - P[:, k]) / d[:, k], -h, h), -h)
            g = _dF(P, d, e, tb)
            up = (g <= 0.0) & (tb > lo)
            lo, glo = np.where(up, tb, lo), np.where(up, g, glo)
            dn = (g >= 0.0) & (tb < hi)
            hi, ghi = np.where(dn, tb, hi), np.where(dn, g, ghi)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ghi > glo, lo + (hi - lo) * (-glo / (ghi - glo)), lo)
    t = np.where(at_lo, -h, np.where(at_hi, h, t))
    p = P + t[:, None] * d
    return np.linalg.norm(p - np.clip(p, -e, e), axis=-1)


def capsule_box(cp, cm, cs, bp, bm, be, margin):
    """dist = d_seg - r: one contact; a segment inside the box has d_seg = 0."""
    cp, cs, bp, be = _a(cp, 3), _a(cs, 3), _a(bp, 3), _a(be, 3)
    P = to_frame(bm, cp - bp)
    d = to_frame(bm, zcol(cm))
    return _tally((seg_box_dist(P, d, be, cs[:, 1]) - cs[:, 0])[:, None], margin)


def collide(t1, p1, m1, s1, t2, p2, m2, s2, margin):
    """N pairs of one capsule pair type, geom 1 first by (type, model index) as sspd::collide."""
    if t1 == PLANE and t2 == CAPSULE:
        return plane_capsule(p1, m1, p2, m2, s2, margin)
    if t1 == SPHERE and t2 == CAPSULE:
        return sphere_capsule(p1, _a(s1, 3)[:, 0], p2, m2, s2, margin)
    if t1 == CAPSULE and t2 == CAPSULE:
        return capsule_capsule(p1, m1, s1, p2, m2, s2, margin)
    if t1 == CAPSULE and t2 == BOX:
        return capsule_box(p1, m1, s1, p2, m2, s2, margin)
    raise ValueError("not a supported capsule pair: %d, %d" % (t1, t2))


def decisive_gap(dists, margin):
    """How far each pair's decisions are from flipping: the least |dist - threshold| over the
    tests it ran."""
    margin = np.asarray(margin, float).reshape(-1, 1)
    g = np.minimum(np.abs(dists - margin), np.abs(dists - DEEP))
    return np.nanmin(g, 1)


# ------------------------------------------------------------------ independent distances
def point_seg_independent(x, c, a, h):
    """Distance of x to the segment c +- h a (|a| = 1): the distance to the line where the foot
    lies inside the segment, to the nearer end otherwise."""
    w = x - c
    t = dot(a, w)
    line = np.linalg.norm(np.cross(a, w), axis=-1)
    end = np.linalg.norm(w - np.sign(t)[:, None] * h[:, None] * a, axis=-1)
    return np.where(np.abs(t) <= h, line, end)


def seg_seg_independent(p1, a1, h1, p2, a2, h2):
    """min over the lines' common perpendicular (where its feet lie inside both segments) and
    the four end-to-segment distances."""
    best = np.minimum.reduce([point_seg_independent(p1 + h1[:, None] * a1, p2, a2, h2),
                              point_seg_independent(p1 - h1[:, None] * a1, p2, a2, h2),
                              point_seg_independent(p2 + h2[:, None] * a2, p1, a1, h1),
                              point_seg_independent(p2 - h2[:, None] * a2, p1, a1, h1)])
    n = np.cross(a1, a2)
    nn = dot(n, n)
    w = p2 - p1
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = dot(np.cross(w, a2), n) / nn
        t2 = dot(np.cross(w, a1), n) / nn
        perp = np.abs(dot(w, n)) / np.sqrt(nn)
    inside = (nn > 1e-24) & (np.abs(t1) <= h1) & (np.abs(t2) <= h2)
    return np.where(inside, np.minimum(best, perp), best)


def point_box(p, e):
    return np.linalg.norm(p - np.clip(p, -e, e), axis=-1)


def seg_box_independent(P, d, e, h, n=129):
    """Dense sampling of t, then golden-section refinement of the convex f(t) = dist(P + t d,
    box) on the bracket around the best sample."""
    ts = np.linspace(-1.0, 1.0, n)[None, :] * h[:, None]                    # [N, n]
    f = point_box(P[:, None, :] + ts[:, :, None] * d[:, None, :], e[:, None, :])
    i = np.argmin(f, 1)
    rows = np.arange(len(h))
    lo, hi = ts[rows, np.maximum(i - 1, 0)], ts[rows, np.minimum(i + 1, n - 1)]
    g = (np.sqrt(5.0) - 1.0) / 2.0
    fun = lambda t: point_box(P + t[:, None] * d, e)
    c, dd = hi - g * (hi - lo), lo + g * (hi - lo)
    fc, fd = fun(c), fun(dd)
    for _ in range(90):
        left = fc < fd
        hi, lo = np.where(left, dd, hi), np.where(left, lo, c)
        c, dd = hi - g * (hi - lo), lo + g * (hi - lo)
        fc, fd = fun(c), fun(dd)
    return np.minimum(np.minimum(fc, fd), f[rows, i])
