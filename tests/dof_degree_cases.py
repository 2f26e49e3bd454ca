"""Cases for every (dof, degree) instantiation of the sampling planner's kernels, and an
independent arc-length reference — TEST INFRASTRUCTURE ONLY (CPU; no GPU, no product code).

k_sspp_c2f and k_sspp_census exist once per D in {1, 2, 3, 4, 6, 7, 9} and p in {2, 3}.  This
module names the cases tests/test_gpu_dof_degree.py runs on the device and
tests/test_dof_degree_cases.py checks on the CPU: the scenes (a window whose qpos0 quaternion is
not the identity, so a window that ends before or inside the quaternion rotates the mover), the
(D, p, n) lists with their sigmas, the knot kinds, and arc_ref, a long-double Cox-de Boor chord
sum that shares no code with oracle/ or the product.
"""
import os

import numpy as np

from oracle import mjcf_ref
from oracle import oracle as O
from tests import synth_scenes as Y

DOFS = (1, 2, 3, 4, 6, 7, 9)
DEGREES = (2, 3)
SEED = 7
B, W = 256, 33
FIRST = 2 ** 40 + 5          # candidate ids above 2^32: Philox's high counter word is not zero
MIN_EACH = 8                 # candidates of either outcome every scene case needs

# ------------------------------------------------------------------ scenes
_Q = np.array([0.9, 0.1, -0.2, 0.3])
Q0 = _Q / np.linalg.norm(_Q)  # the mover's qpos0 quaternion, as both loaders normalise it
WIN_LIMITS = np.array([1, 1, 1, .3, .3, .3, .3])
TWO_LIMITS = np.array([1, 1, 1, .3, .3, .3, .3, 1, 1])


def _window(one_geom, cylinder=True):
    statics = [Y.ramp(),
               # beyond the path's end: a D = 1 candidate reaches it only by overshooting in x
               Y.geom(Y.SPHERE, 0.05, (0.66, 0, 0.3), name="stop"),
               Y.geom(Y.BOX, (0.05, 0.03, 0.04), (0.25, 0.15, 0.3), (0.8, 0.1, 0.5, 0.3), name="brick")]
    if cylinder:
        statics.append(Y.geom(Y.CYLINDER, (0.04, 0.06), (0.3, -0.02, 0.47), name="post"))
    geoms = [Y.geom(Y.BOX, Y.MOVER_BOX, name="m_box")]
    if not one_geom:
        geoms.append(Y.geom(Y.SPHERE, 0.03, (0.07, 0, 0.01), name="m_ball"))
    return Y.mjcf(statics, [Y.body("mover", (0, 0, 0.3), geoms, quat=_Q)])


def window():
    """One free body (a box and an offset sphere) whose qpos0 quaternion is not the identity,
    over the tilted plane, a sphere past the path's end, a rotated box and a vertical cylinder."""
    return _window(False)


def window_one():
    """window() with the mover's box only: a one-geom mover."""
    return _window(True)


def window_one_nocyl():
    """window_one() without the cylinder: no cylinder-box pair, so a multi-step launch splits."""
    return _window(True, cylinder=False)


SCENES = {"window": window, "window_one": window_one, "window_one_nocyl": window_one_nocyl,
          "two_movers": Y.two_movers}


def scene_name(D):
    return "two_movers" if D == 9 else "window"


def write_scene(root, name):
    path = os.path.join(str(root), name + ".xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(SCENES[name]())
    return path


_oscenes = {}


def oracle_scene(root, name, D):
    """The oracle's scene `name` bound to a qpos window of D, loaded once."""
    key = (str(root), name, D)
    if key not in _oscenes:
        _oscenes[key] = O.Scene(mjcf_ref.load(write_scene(root, name)), 0, D)
    return _oscenes[key]


def ends(D):
    """(start, end, limits) of the path of dof D."""
    if D == 9:
        # TWO_START -> TWO_END at their z = 0.25 runs through body 1, so the initial spline
        # collides at every (p, n) and lowering sigma leaves nothing feasible: the path is
        # raised to z = 0.36, where the straight line is free and the candidates dip into
        # the statics and body 1
        s, e = Y.TWO_START.copy(), Y.TWO_END.copy()
        s[2] = e[2] = 0.36
        return s, e, TWO_LIMITS.copy()
    s = np.concatenate([[0.0, 0.0, 0.3], Q0])
    e = np.concatenate([[0.5, 0.0, 0.3], Q0])
    return s[:D].copy(), e[:D].copy(), WIN_LIMITS[:D].copy()


def init_spline(D, p, n):
    """initializePath for degree p: the spline through n points of the straight line (the
    oracle's interpolation, which the product's equals bit for bit)."""
    s, e, _ = ends(D)
    u = np.array([i / (n - 1) for i in range(n)])
    return O.interpolate(np.array([(1 - t) * s + t * e for t in u]), p, u)


def npert(D, p, n):
    """Perturbed entries of a sampled candidate: rows p .. n - p - 1."""
    return max(0, n - 2 * p) * D


def sigma_for(D):
    # D = 1 at 0.12 is nearly all feasible; the two-mover scene is crowded: at 0.15 degree 2
    # with n = 10 keeps 6 feasible of 256, at 0.08 every D = 9 case keeps 41 to 172
    return {1: 0.25, 9: 0.08}.get(D, 0.12)


# ------------------------------------------------------------------ case lists
def matrix_cases():
    """(a): (D, p, n) with one perturbed row, two rows, several.  n = 2p + 1 with odd D: odd npert."""
    out = [(D, p, n) for D in DOFS[:-1] for p in DEGREES for n in (2 * p + 1, 2 * p + 2, 10)]
    return out + [(9, p, n) for p in DEGREES for n in (2 * p + 1, 10)]


FP32_CASES = [(1, 2, 5), (3, 2, 5), (3, 3, 8), (7, 3, 7), (9, 2, 6)]   # npert 1, 3, 6, 7, 18

NOPERT_B, NOPERT_SIGMA = 300, 0.2
NOPERT_FIRST = 2 ** 33 - 100   # the batch's ids straddle a multiple of 2^32


def nopert_cases():
    """(c): (D, p, n, with_scene), n in {p + 1, 2p}: no perturbed row."""
    return [(D, p, n, sc) for D in (1, 4, 9) for p in DEGREES for n in (p + 1, 2 * p) for sc in (False, True)]


KNOT_KINDS = ("uniform", "random", "double", "grid")
W_LIST = (2, 3, 64, 65, 66, 129, 130, 193, 194, 257, 258, 1025)
N_SPLINES = 64


def knot_vector(n, p, kind, rng):
    """A clamped knot vector on [0, 1] with n - p - 1 interior knots."""
    m = n - p - 1
    if kind == "uniform":
        inner = np.array([(i + 1) / (m + 1) for i in range(m)])
    elif kind in ("random", "double"):
        inner = np.sort(rng.uniform(0.02, 0.98, size=m))
        if kind == "double":
            assert m >= 2
            inner[1] = inner[0]
    elif kind == "grid":
        # on the collision parameters i / 16 (W = 16) and the arc parameters i / 16 (W = 17)
        inner = np.sort(rng.choice(np.arange(1, 16), size=m, replace=m > 15)) / 16.0
    else:
        raise ValueError(kind)
    return np.concatenate([np.zeros(p + 1), inner, np.ones(p + 1)])


def knot_cases():
    """(d): (D, p, n, kind, W) for every (D, p).  n = p + 1 has no interior knot (every kind is
    the Bezier vector) and `double` needs two, so the kinds meet the sizes that can hold them.
    W cycles through W_LIST per degree, so every W meets every degree; grid takes 16 and 17."""
    out = []
    for p in DEGREES:
        k = g = 0
        for D in DOFS:
            for n, kind in ((p + 1, "uniform"), (p + 2, "random"), (p + 2, "grid"), (2 * p + 1, "double"),
                            (2 * p + 1, "uniform"), (2 * p + 1, "grid"), (13, "uniform"), (13, "random"),
                            (13, "double"), (13, "grid")):
                if kind == "grid":
                    out.append((D, p, n, kind, (16, 17)[g % 2]))
                    g += 1
                else:
                    out.append((D, p, n, kind, W_LIST[k % len(W_LIST)]))
                    k += 1
    return out


def knot_case_data(D, p, n, kind, W_):
    """(knots, ctrl [64][n][D]) of a (d) case, from the case's own seed."""
    rng = np.random.default_rng([D, p, n, KNOT_KINDS.index(kind), W_])
    knots = knot_vector(n, p, kind, rng)
    return knots, rng.normal(0.0, 1.0, size=(N_SPLINES, n, D))


W1_CASES = [(3, 2), (7, 3)]
W1_B, W1_N = 128, 7


def w1_ctrl(D, p):
    """(e): caller splines whose end rows (the only waypoints W = 1 checks) are perturbed."""
    knots, ctrl0 = init_spline(D, p, W1_N)
    _, _, lim = ends(D)
    rng = np.random.default_rng([1, D, p])
    ctrl = np.repeat(ctrl0[None], W1_B, axis=0)
    ctrl[:, 0] += rng.normal(0, 0.1, size=(W1_B, D)) * lim
    ctrl[:, -1] += rng.normal(0, 0.1, size=(W1_B, D)) * lim
    return knots, ctrl0, ctrl


def w1_expected(root, D, p):
    """W = 1 checks u = 0 and u = 1 only; the oracle's scorer refuses W < 2, so by hand."""
    knots, ctrl0, ctrl = w1_ctrl(D, p)
    osc = oracle_scene(root, "window", D)
    feas = np.array([osc.contacts(O.spline_eval(knots, p, c, 0.0))[0] == 0 and
                     osc.contacts(O.spline_eval(knots, p, c, 1.0))[0] == 0 for c in ctrl], np.uint8)
    return knots, ctrl0, ctrl, feas


SPLIT_CASES = [(3, 2), (4, 3)]
SPLIT_STEPS, SPLIT_B, SPLIT_N = 16, 1024, 10
SPLIT_FIRST = 2 ** 32 - 3 * 1024   # step 3 starts at 2^32

DROPIN_SEED = 0x5EED   # the drop-in planner's default seed
DROPIN = dict(sample_count=256, check_points=32, init_points=9)


# ------------------------------------------------------------------ the independent reference
LD = np.longdouble


def basis_matrix(knots, p, u):
    """Cox-de Boor in long double: N[i, j] = N_{j, p}(u[i]) by the recursive definition, spans
    half open [t_j, t_j+1) and the last non-empty span closed at u = 1; 0 / 0 = 0."""
    t = np.asarray(knots, dtype=LD)
    u = np.asarray(u, dtype=LD)
    m = len(t) - 1
    last = max(j for j in range(m) if t[j] < t[j + 1])
    N = np.zeros((len(u), m), dtype=LD)
    for j in range(m):
        inside = (t[j] <= u) & (u < t[j + 1])
        if j == last:
            inside |= u == t[j + 1]
        N[:, j] = inside
    for d in range(1, p + 1):
        M = np.zeros((len(u), m - d), dtype=LD)
        for j in range(m - d):
            if t[j + d] > t[j]:
                M[:, j] += (u - t[j]) / (t[j + d] - t[j]) * N[:, j]
            if t[j + d + 1] > t[j + 1]:
                M[:, j] += (t[j + d + 1] - u) / (t[j + d + 1] - t[j + 1]) * N[:, j + 1]
        N = M
    return N


def arc_params(W_):
    """The arc-length grid: the doubles i / (W - 1)."""
    return np.array([i / (W_ - 1) for i in range(W_)])


def arc_ref(knots, p, ctrl, W_):
    """Chord sum of the spline(s) ctrl [..., n, D] on W points, in long double."""
    N = basis_matrix(knots, p, arc_params(W_))
    pts = np.einsum("wn,...nd->...wd", N, np.asarray(ctrl, dtype=LD))
    d = pts[..., 1:, :] - pts[..., :-1, :]
    return np.sqrt((d * d).sum(axis=-1)).sum(axis=-1)


def oracle_vs_ref(cases=None):
    """The oracle's largest relative deviation from arc_ref over the (d) cases."""
    worst = 0.0
    for D, p, n, kind, W_ in (knot_cases() if cases is None else cases):
        knots, ctrl = knot_case_data(D, p, n, kind, W_)
        arc_o, _ = O.sspp_score(None, knots, p, ctrl, W_, arc_all=True)
        ref = arc_ref(knots, p, ctrl, W_)
        worst = max(worst, float(np.max(np.abs(arc_o.astype(LD) - ref) / ref)))
    return worst


def ref_bar(measured):
    """The device's bar against arc_ref: 16 x the oracle's own deviation, at least 1e-12."""
    return max(1e-12, 16.0 * measured)
