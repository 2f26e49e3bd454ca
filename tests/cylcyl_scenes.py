"""Cylinder-cylinder scenes and their reference scoring — TEST INFRASTRUCTURE ONLY.

The CPU oracle knows no cylinder-cylinder pair (its collide returns -1 for one), so the reference
score of a scene is composed, as for capsules (tests/capsule_scenes.py): the oracle on a copy of
the scene in which the collision bits that only cylinder-cylinder pairs use are cleared, plus
tests/cylcyl_ref.py on the cylinder-cylinder pairs, with world poses from the oracle's forward
kinematics.  Bits: static cylinders carry bit 4 only, a mover cylinder 1 | 4 (so it also meets the
planes and boxes, which carry bit 1), the resting pair of the static-contact scene bit 8; the
oracle's copy clears 4 and 8 everywhere.
"""
import numpy as np

from oracle import oracle as O
from tests import capsule_scenes as CS
from tests import cylcyl_ref as R
from tests import synth_scenes as Y

CYL = Y.CYLINDER
CC_BITS = 4 | 8
START, END, LIMITS, SIGMA = CS.START, CS.END, CS.LIMITS, CS.SIGMA


def post(r, h, pos, quat=(1.0, 0.0, 0.0, 0.0), name="", bit=4, **kw):
    """a static cylinder that only cylinders with the same bit meet"""
    return Y.geom(CYL, (r, h), pos, quat, name=name, contype=bit, conaffinity=bit, **kw)


def mover_cyl(r, h, pos=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0), name="m_cyl", **kw):
    return Y.geom(CYL, (r, h), pos, quat, name=name, contype=5, conaffinity=5, **kw)


# ------------------------------------------------------------------ SamplingPathPlanner scenes
def sspp_cyl_mover():
    """(i) a cylinder mover against a vertical and a tilted static cylinder, the tilted plane and a box"""
    st = [Y.ramp(),
          post(0.04, 0.1, (0.14, 0.11, 0.2), name="v0"),
          post(0.035, 0.1, (0.3, -0.1, 0.22), (0.92, 0.3, 0.2, 0.1), name="t0"),
          Y.geom(Y.BOX, (0.05, 0.06, 0.04), (0.44, 0.07, 0.27), (0.8, 0.1, 0.5, 0.3), name="slab")]
    return st, [Y.body("mover", (0, 0, 0.3), [mover_cyl(0.03, 0.045, quat=(0.8, 0.0, 0.6, 0.0), margin=0.002)])]


def _two_geom_mover():
    return Y.body("mover", (0, 0, 0.3), [Y.geom(Y.BOX, Y.MOVER_BOX, name="m_box"),
                                          mover_cyl(0.02, 0.04, (0.0, 0.0, -0.045), (0.7, 0.7, 0.0, 0.1))])


def sspp_two_geom_mover():
    """(ii) a box + cylinder mover (ONEGEOM false) in a table with box-box pairs: 7 pairs"""
    st = [Y.ramp()] + Y.one_type_statics("boxes")[:2] + [post(0.035, 0.09, (0.27, 0.02, 0.05), (0.7, 0.1, 0.7, 0.0), name="t0")]
    return st, [_two_geom_mover()]


def sspp_ten_pairs():
    """(iii) the same mover against three boxes and two static cylinders: 10 pairs (hull masks)"""
    st = [Y.ramp()] + Y.one_type_statics("boxes") + [post(0.035, 0.09, (0.27, 0.02, 0.05), (0.7, 0.1, 0.7, 0.0), name="t0"),
                                                     post(0.03, 0.08, (0.4, -0.12, 0.14), name="v0")]
    return st, [_two_geom_mover()]


def sspp_static_contact():
    """(iv) scene (i) plus two cylinders 5 mm into each other that are static for the planner: one
    in the world, one on a second free body outside the qpos window (bit 8: they meet only each
    other)."""
    st, bodies = sspp_cyl_mover()
    st = st + [post(0.05, 0.03, (0.9, 0.4, 0.3), name="drum", bit=8)]
    rest = Y.body("rest", (0.9, 0.4, 0.345), [post(0.02, 0.05, (0, 0, 0), (0.7071, 0.0, 0.7071, 0.0), name="pin", bit=8)])
    return st, bodies + [rest]


# ------------------------------------------------------------------ TaskSpacePlanner scenes
def tsp_gripper(tilted=False):
    """A gripper-like mover (a box and a vertical cylinder, as robocrane's col_mount) among vertical
    posts, an upright box and the floor; `tilted` tilts one post, which takes the generic kernels."""
    q = (0.92, 0.3, 0.2, 0.1) if tilted else (1.0, 0.0, 0.0, 0.0)
    st = [Y.geom(Y.PLANE, (0, 0, 1), name="floor"),
          post(0.04, 0.12, (0.0, 0.1, 0.14), name="p0"),
          post(0.03, 0.15, (0.1, -0.1, 0.16), q, name="p1"),
          post(0.05, 0.08, (0.22, 0.04, 0.3), name="p2"),
          Y.geom(Y.BOX, (0.04, 0.05, 0.08), (-0.1, -0.12, 0.1), (0.9239, 0, 0, 0.3827), name="b0")]
    mover = Y.body("mover", (-0.3, 0, 0.2), [Y.geom(Y.BOX, (0.03, 0.02, 0.015), (0, 0, -0.04), name="m_box"),
                                              mover_cyl(0.025, 0.03, name="m_cyl")])
    return st, [mover]


# ------------------------------------------------------------------ composed reference
def oracle_copy(ref):
    """the scene without the bits cylinder-cylinder pairs meet on; no such pair may be left"""
    m = dict(ref)
    m["geom_contype"] = np.asarray(ref["geom_contype"]) & ~CC_BITS
    m["geom_conaffinity"] = np.asarray(ref["geom_conaffinity"]) & ~CC_BITS
    assert not cc_pairs(m, set(range(len(ref["body_parent"]))))
    return m


def cc_pairs(ref, moving_bodies):
    """The collidable cylinder-cylinder pairs with a moving geom (product filter rules), geom 1 the
    lower model index: (g1, g2, margin)."""
    gb, gt = ref["geom_body"], ref["geom_type"]
    ct, ca = ref["geom_contype"], ref["geom_conaffinity"]
    out = []
    for g1 in range(len(gb)):
        for g2 in range(g1 + 1, len(gb)):
            if gb[g1] == gb[g2] or not (gb[g1] in moving_bodies or gb[g2] in moving_bodies):
                continue
            if not ((ct[g1] & ca[g2]) or (ct[g2] & ca[g1])) or gt[g1] != CYL or gt[g2] != CYL:
                continue
            out.append((g1, g2, max(ref["geom_margin"][g1], ref["geom_margin"][g2])))
    return out


def pair_sd(ref, pairs, xp, xm, deep=False):
    """per pair: (signed distance [N] where the decision against the pair's margin — deep: against
    -1e-3 — needs it (tests/cylcyl_ref.scene_sd), centre distance [N])"""
    size = np.asarray(ref["geom_size"], float)
    out = []
    for g1, g2, mg in pairs:
        assert mg >= 0.0
        d, _ = R.scene_sd(xp[:, g2] - xp[:, g1], xm[:, g1][:, [2, 5, 8]], size[g1][0], size[g1][1],
                          xm[:, g2][:, [2, 5, 8]], size[g2][0], size[g2][1], R.DEEP if deep else mg)
        out.append((d, np.linalg.norm(xp[:, g2] - xp[:, g1], axis=1)))
    return out


def static_cc_contacts(ref, oscene, moving_bodies):
    """(contacts, cost) of the static-static cylinder-cylinder pairs at qpos0"""
    gb = ref["geom_body"]
    every = cc_pairs(ref, set(range(len(ref["body_parent"]))))
    stat = [p for p in every if gb[p[0]] not in moving_bodies and gb[p[1]] not in moving_bodies]
    xp, xm = oscene.fk(np.asarray(ref["qpos0"], float)[:oscene.arg])
    n, cost = 0, 0.0
    for (g1, g2, mg), (d, cd), (dd, _) in zip(stat, pair_sd(ref, stat, xp[None], xm[None]),
                                              pair_sd(ref, stat, xp[None], xm[None], deep=True)):
        n += int(d[0] < mg)
        cost += int(dd[0] < R.DEEP) * (-1.0 / (cd[0] + 1e-4))
    return n, cost


def sspp_reference(ref, knots, ctrl, W, dof=7):
    """The composed SamplingPathPlanner reference of `ctrl` [B, n, dof]: dict(feas, arc, hit
    [B, npairs] (a lower bound of each pair's hits where another contact is proven), near [B],
    pairs, feas_nocc).  Feasible = the oracle's feasibility without the
    cylinder-cylinder pairs AND no such pair in contact at any waypoint u = i / W; a candidate with
    a cylinder-cylinder distance within R.BAND of its margin at some waypoint is `near`."""
    occ = O.Scene(oracle_copy(ref), 0, dof)
    movers = {b for b in range(len(ref["body_parent"])) if 0 <= ref["body_qpos_adr"][b] < dof}
    pairs = cc_pairs(ref, movers)
    _, feas_nocc = O.sspp_score(occ, knots, 3, ctrl, W)
    arc_all, _ = O.sspp_score(None, knots, 3, ctrl, W)
    B = len(ctrl)
    hit = np.zeros((B, len(pairs)), bool)
    near = np.zeros(B, bool)
    live = np.flatnonzero(feas_nocc)  # (a candidate the other geoms stop is infeasible already)
    if len(live) and pairs:
        qs = CS.sspp_waypoints(knots, ctrl[live], W).reshape(-1, dof)
        xp, xm = CS.fk_all(occ, qs)
        size = np.asarray(ref["geom_size"], float)
        args = [(xp[:, g2] - xp[:, g1], xm[:, g1][:, [2, 5, 8]], size[g1][0], size[g1][1],
                 xm[:, g2][:, [2, 5, 8]], size[g2][0], size[g2][1], mg) for g1, g2, mg in pairs]
        # the bounds first: a candidate with a contact they prove is infeasible whatever its other
        # waypoints do, so the search runs for the other candidates' undecided waypoints only
        rough = [R.scene_bounds(*a) for a in args]
        sure = np.zeros(len(live), bool)
        for a, (d, todo) in zip(args, rough):
            sure |= (d < a[7]).reshape(len(live), W + 1).any(1)  # (nan compares false)
        for k, (a, (d, todo)) in enumerate(zip(args, rough)):
            d = R.scene_search(d, np.flatnonzero(todo & np.repeat(~sure, W + 1)), *a[:7])
            hit[live, k] = (d < a[7]).reshape(len(live), W + 1).any(1)
            near[live] |= ~sure & (np.abs(d - a[7]) <= R.BAND).reshape(len(live), W + 1).any(1)
    feas = (feas_nocc.astype(bool) & ~hit.any(1)).astype(np.uint8)
    return dict(feas=feas, arc=np.where(feas == 1, arc_all, np.inf), hit=hit, near=near, pairs=pairs,
                feas_nocc=feas_nocc)


def tsp_compose(occ, ref, pairs, start, end, vias, cp, w_collision=1.0):
    """or_tsp_score's composition with the cylinder-cylinder pairs' terms added to each point's
    cost: (L, C_nf, C_wf, status, cost, deep [B, cp, npairs], near [B])."""
    P = CS.tsp_points(start, end, vias, cp)
    B = len(P)
    flat = P[:, 1:].reshape(-1, 4)
    xp, xm = CS.fk_all(occ, flat)
    res = pair_sd(ref, pairs, xp, xm, deep=True)
    extra = np.zeros(len(flat))
    near = np.zeros(len(flat), bool)
    deep = np.zeros((len(flat), len(pairs)), int)
    for k, ((g1, g2, mg), (d, cd)) in enumerate(zip(pairs, res)):
        dp = (d < R.DEEP).astype(int)  # (margins are >= 0 > -1e-3: a deep pair is in contact)
        deep[:, k] = dp
        extra += dp * (-1.0 / (cd + 1e-4))
        near |= np.abs(d - R.DEEP) <= R.BAND
    base = np.array([occ.contacts(q, True)[1] for q in flat])
    c = (base + extra).reshape(B, cp)
    deficit = 0.01 - P[:, 1:, 2]
    fp = np.where(deficit > 0.0, (10.0 * deficit) * deficit, 0.0)
    seg = np.sqrt(((P[:, 1:] - P[:, :-1]) ** 2).sum(-1))
    L = np.array([O.canon_sum(x) for x in seg])
    Cnf = np.array([O.canon_sum(x) for x in c])
    Cwf = np.array([O.canon_sum(x) for x in c + fp])
    return (L, Cnf, Cwf, (Cnf == 0.0).astype(np.uint8), L + w_collision * Cwf, deep.reshape(B, cp, len(pairs)),
            near.reshape(B, cp).any(1))
