"""Capsule scenes and their reference scoring — TEST INFRASTRUCTURE ONLY.

Scenes are authored on top of tests/synth_scenes.py (its geom / body records), with two
additions: the capsule type, and capsules / cylinders written with `fromto`.  The independent
reader (oracle/mjcf_ref.py) reads no `fromto` and the CPU oracle knows no capsule, so

* every scene can be written twice: as authored (the product loads it) and `explicit` (each
  fromto geom restated as pos / quat / size by the loader's documented rule; mjcf_ref loads it);
* the reference score of a scene is composed: the oracle on the scene without its capsules
  (skip_types=(3,)) plus tests/capsule_ref.py on the capsule pairs, with world poses from the
  oracle's forward kinematics (which ignores geom types).
"""
import numpy as np

from oracle import oracle as O
from tests import capsule_ref as R
from tests import synth_scenes as Y

CAPSULE = 3
_TYPE_NAMES = dict(Y._TYPE_NAMES)
_TYPE_NAMES[CAPSULE] = "capsule"


# ------------------------------------------------------------------ rotations
def quat_z_to(d):
    """The loader's fromto rule: the shortest rotation taking +z to d (normalised), as
    (1 + d_z, -d_y, d_x, 0) normalised; the rotation by pi about x when d = -z."""
    d = np.asarray(d, float)
    d = d / np.linalg.norm(d)
    s2 = d[0] * d[0] + d[1] * d[1]
    if d[2] < 0.0 and s2 == 0.0:
        return np.array([0.0, 1.0, 0.0, 0.0])
    w = 1.0 + d[2] if d[2] >= 0.0 else s2 / (1.0 - d[2])
    q = np.array([w, -d[1], d[0], 0.0])
    return q / np.linalg.norm(q)


def quat2mat(q):
    """Row-major 3x3 (flat 9) of a quaternion, normalised first."""
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z])


# ------------------------------------------------------------------ authoring
def capsule(r, h, pos=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0), **kw):
    return Y.geom(CAPSULE, (r, h), pos, quat, **kw)


def fromto(type, r, a, b, **kw):
    """A capsule / cylinder written as fromto="a b" size="r"."""
    g = Y.geom(type, (r,), **kw)
    g["fromto"] = tuple(float(x) for x in a) + tuple(float(x) for x in b)
    return g


def explicit(g):
    """A fromto geom restated with pos / quat / size (the loader's rule)."""
    if "fromto" not in g:
        return g
    a, b = np.array(g["fromto"][:3]), np.array(g["fromto"][3:])
    e = {k: v for k, v in g.items() if k != "fromto"}
    e["pos"] = tuple(0.5 * (a + b))
    e["size"] = (g["size"][0], 0.5 * float(np.linalg.norm(b - a)))
    e["quat"] = tuple(quat_z_to(b - a))
    return e


def _geom_xml(g):
    if "fromto" in g:
        s = '<geom type="%s" size="%s" fromto="%s"' % (_TYPE_NAMES[g["type"]], Y._vec(g["size"][:1]), Y._vec(g["fromto"]))
    else:
        s = '<geom type="%s" size="%s" pos="%s" quat="%s"' % (_TYPE_NAMES[g["type"]], Y._vec(g["size"]),
                                                              Y._vec(g["pos"]), Y._vec(g["quat"]))
    if g["name"]:
        s += ' name="%s"' % g["name"]
    if g["contype"] != 1:
        s += ' contype="%d"' % g["contype"]
    if g["conaffinity"] != 1:
        s += ' conaffinity="%d"' % g["conaffinity"]
    if g["margin"]:
        s += ' margin="%s"' % repr(g["margin"])
    return s + "/>"


def mjcf(statics, bodies, as_explicit=False):
    """Y.mjcf with capsules and fromto; as_explicit: every fromto geom restated."""
    f = explicit if as_explicit else (lambda g: g)
    out = ['<mujoco>', '  <compiler angle="radian"/>', '  <worldbody>']
    out += ["    " + _geom_xml(f(g)) for g in statics]
    for b in bodies:
        out.append('    <body name="%s" pos="%s" quat="%s">' % (b["name"], Y._vec(b["pos"]), Y._vec(b["quat"])))
        out.append('      <freejoint/>')
        out += ["      " + _geom_xml(f(g)) for g in b["geoms"]]
        out.append('    </body>')
    out += ['  </worldbody>', '</mujoco>']
    return "\n".join(out) + "\n"


# ------------------------------------------------------------------ SamplingPathPlanner scenes
START = np.array([0.0, 0.0, 0.16, 1, 0, 0, 0])
END = np.array([0.5, 0.0, 0.16, 1, 0, 0, 0])
LIMITS = Y.ZOO_LIMITS
SIGMA = 0.12


def sspp_capsule_mover():
    """(i) a capsule mover against the tilted plane and a static sphere, capsule and box."""
    st = [Y.ramp(),
          Y.geom(Y.SPHERE, 0.06, (0.12, 0.13, 0.2), name="ball"),
          capsule(0.03, 0.09, (0.27, -0.12, 0.22), (0.9, 0.3, -0.2, 0.1), name="rod"),
          Y.geom(Y.BOX, (0.05, 0.06, 0.04), (0.42, 0.06, 0.27), (0.8, 0.1, 0.5, 0.3), name="slab")]
    mover = Y.body("mover", (0, 0, 0.3), [capsule(0.025, 0.05, quat=(0.8, 0.0, 0.6, 0.0), name="m_cap", margin=0.002)])
    return st, [mover]


def sspp_static_capsules():
    """(ii) a box mover and a sphere mover geom against static capsules, two written with fromto."""
    st = [Y.ramp(),
          capsule(0.03, 0.1, (0.1, 0.14, 0.2), (0.9, 0.3, 0.2, 0.1), name="c0"),
          fromto(CAPSULE, 0.025, (0.2, -0.2, 0.12), (0.3, -0.08, 0.32), name="c1"),
          fromto(CAPSULE, 0.035, (0.42, 0.12, 0.48), (0.42, -0.02, 0.34), name="c2")]
    mover = Y.body("mover", (0, 0, 0.3), [Y.geom(Y.BOX, Y.MOVER_BOX, name="m_box"),
                                          Y.geom(Y.SPHERE, 0.03, (0.0, 0.0, 0.07), name="m_ball")])
    return st, [mover]


def sspp_two_geom_mover():
    """(iii) a two-geom mover (capsule + box) in a table that also holds box-box pairs: the
    filtered scan beside capsule pairs that only FP64 decides."""
    st = [Y.ramp()] + Y.one_type_statics("boxes") + [capsule(0.03, 0.08, (0.25, 0.0, 0.035), (0.7, 0.1, 0.7, 0.0), name="rod")]
    mover = Y.body("mover", (0, 0, 0.3), [Y.geom(Y.BOX, Y.MOVER_BOX, name="m_box"),
                                          capsule(0.02, 0.05, (0.0, 0.0, -0.045), (0.7, 0.7, 0.0, 0.1), name="m_cap")])
    return st, [mover]


def sspp_static_contact():
    """(iv) scene (ii) with a capsule resting 5 mm in a box, both static for the planner: the
    box in the world, the capsule on a second free body outside the qpos window (geoms of one
    body never collide, the world's included, so an env-env contact needs two bodies)."""
    st, bodies = sspp_static_capsules()
    st = st + [Y.geom(Y.BOX, (0.05, 0.05, 0.03), (0.9, 0.4, 0.3), name="tray")]
    rest = Y.body("rest", (0.9, 0.4, 0.345), [capsule(0.02, 0.06, quat=(0.7071, 0.0, 0.7071, 0.0), name="pin")])
    return st, bodies + [rest]


# ------------------------------------------------------------------ TaskSpacePlanner scenes
def tsp_capsule_mover():
    """A vertical capsule mover (yaw keeps it exactly vertical) among vertical static capsules
    (the parallel branch), a tilted capsule, boxes and the floor plane."""
    st = [Y.geom(Y.PLANE, (0, 0, 1), name="floor"),
          capsule(0.04, 0.1, (0.0, 0.1, 0.2), name="v0"),
          capsule(0.03, 0.12, (0.12, -0.1, 0.2), name="v1"),
          capsule(0.035, 0.1, (0.22, 0.08, 0.24), (0.92, 0.3, 0.2, 0.1), name="t0"),
          Y.geom(Y.BOX, (0.04, 0.05, 0.08), (-0.1, -0.12, 0.1), (0.9239, 0, 0, 0.3827), name="b0"),
          Y.geom(Y.BOX, (0.05, 0.04, 0.05), (0.3, -0.2, 0.15), (0.8, 0.1, 0.5, 0.3), name="b1")]
    return st, [Y.body("mover", (-0.3, 0, 0.2), [capsule(0.03, 0.06, name="m_cap")])]


def tsp_box_mover():
    """A box mover among capsules (vertical, tilted, one by fromto) over the floor plane."""
    st = [Y.geom(Y.PLANE, (0, 0, 1), name="floor"),
          capsule(0.04, 0.1, (0.0, 0.11, 0.2), name="v0"),
          capsule(0.035, 0.12, (0.08, -0.11, 0.2), (0.92, 0.3, 0.2, 0.1), name="t0"),
          fromto(CAPSULE, 0.04, (0.2, -0.05, 0.12), (0.26, 0.1, 0.3), name="f0")]
    return st, [Y.body("mover", (-0.3, 0, 0.2), [Y.geom(Y.BOX, (0.03, 0.03, 0.03), name="m_box")])]


def tsp_no_capsule():
    """The grid check: a capsule-free scene on which the composed reference is the oracle's."""
    return Y.tsp_boxes()


# ------------------------------------------------------------------ composed reference
def capsule_pairs(ref, moving_bodies):
    """The collidable pairs with a capsule in them and a moving geom, product filter rules (bit
    filter, same body; the scenes' bodies all hang off the world), each ordered first-by-(type,
    index) as sspd::collide takes them: (g1, g2, margin)."""
    gb, gt = ref["geom_body"], ref["geom_type"]
    ct, ca = ref["geom_contype"], ref["geom_conaffinity"]
    out = []
    for g1 in range(len(gb)):
        for g2 in range(g1 + 1, len(gb)):
            if gb[g1] == gb[g2] or not (gb[g1] in moving_bodies or gb[g2] in moving_bodies):
                continue
            if not ((ct[g1] & ca[g2]) or (ct[g2] & ca[g1])):
                continue
            if CAPSULE not in (gt[g1], gt[g2]):
                continue
            a, b = (g1, g2) if gt[g1] <= gt[g2] else (g2, g1)
            out.append((a, b, max(ref["geom_margin"][g1], ref["geom_margin"][g2])))
    return out


def static_capsule_contacts(ref, oscene, moving_bodies):
    """Contacts of the static-static pairs with a capsule in them, at qpos0 (mode 0 scenes)."""
    gb = ref["geom_body"]
    every = capsule_pairs(ref, set(range(len(ref["body_parent"]))))
    stat = [p for p in every if gb[p[0]] not in moving_bodies and gb[p[1]] not in moving_bodies]
    xp, xm = oscene.fk(np.asarray(ref["qpos0"], float)[:oscene.arg])
    n = 0
    for g1, g2, mg in stat:
        nc, _, _ = R.collide(ref["geom_type"][g1], xp[g1], xm[g1], ref["geom_size"][g1],
                             ref["geom_type"][g2], xp[g2], xm[g2], ref["geom_size"][g2], mg)
        n += int(nc[0])
    return n


def fk_all(oscene, qs):
    """World geom poses at every configuration: ([N, ngeom, 3], [N, ngeom, 9])."""
    xp = np.empty((len(qs), oscene.ngeom, 3))
    xm = np.empty((len(qs), oscene.ngeom, 9))
    for i, q in enumerate(qs):
        xp[i], xm[i] = oscene.fk(q)
    return xp, xm


def pair_results(ref, pairs, xp, xm):
    """capsule_ref on every capsule pair at every configuration: per pair (contacts [N], deep [N],
    dists [N, k], centre distance [N])."""
    out = []
    size = np.asarray(ref["geom_size"], float)
    for g1, g2, mg in pairs:
        n = len(xp)
        nc, nd, d = R.collide(ref["geom_type"][g1], xp[:, g1], xm[:, g1], np.broadcast_to(size[g1], (n, 3)),
                              ref["geom_type"][g2], xp[:, g2], xm[:, g2], np.broadcast_to(size[g2], (n, 3)), mg)
        out.append((nc, nd, d, np.linalg.norm(xp[:, g2] - xp[:, g1], axis=1)))
    return out


def sspp_waypoints(knots, ctrl, W):
    """checkCollision's configurations: O.spline_eval at u = i / W, i = 0..W, per candidate."""
    return np.array([[O.spline_eval(knots, 3, c, i / W) for i in range(W + 1)] for c in ctrl])


def tsp_points(start, end, vias, cp):
    """eval_one_pass's configurations per candidate: the degree-2 interpolation of [start, vias,
    end] at u_i = i / (n - 1), evaluated at u = i / cp, i = 0..cp."""
    out = []
    for v in vias:
        pts = np.vstack([start, v.reshape(-1, 4), end])
        n = len(pts)
        knots, ctrl = O.interpolate(pts, 2, np.array([i / (n - 1) for i in range(n)]))
        du = 1.0 / cp
        out.append([O.spline_eval(knots, 2, ctrl, i * du) for i in range(cp + 1)])
    return np.array(out)


def tsp_compose(oscene_nocap, ref, pairs, start, end, vias, cp, w_collision=1.0):
    """or_tsp_score's composition with the capsule pairs' terms added to each point's cost:
    returns (L, C_nf, C_wf, status, cost, deep [B, cp, npairs], gap [B, cp])."""
    P = tsp_points(start, end, vias, cp)
    B = len(P)
    flat = P[:, 1:].reshape(-1, 4)
    xp, xm = fk_all(oscene_nocap, flat)
    res = pair_results(ref, pairs, xp, xm)
    cap = np.zeros(len(flat))
    for nc, nd, d, cd in res:
        cap += nd * (-1.0 / (cd + 1e-4))
    base = np.array([oscene_nocap.contacts(q, True)[1] for q in flat])
    gap = np.full(len(flat), np.inf)
    for (g1, g2, mg), (nc, nd, d, cd) in zip(pairs, res):
        gap = np.minimum(gap, R.decisive_gap(d, mg))
    c = (base + cap).reshape(B, cp)
    deficit = 0.01 - P[:, 1:, 2]
    fp = np.where(deficit > 0.0, (10.0 * deficit) * deficit, 0.0)
    seg = np.sqrt(((P[:, 1:] - P[:, :-1]) ** 2).sum(-1))
    L = np.array([O.canon_sum(x) for x in seg])
    Cnf = np.array([O.canon_sum(x) for x in c])
    Cwf = np.array([O.canon_sum(x) for x in c + fp])
    deep = np.stack([r[1] for r in res], 1).reshape(B, cp, len(pairs)) if pairs else np.zeros((B, cp, 0), int)
    return L, Cnf, Cwf, (Cnf == 0.0).astype(np.uint8), L + w_collision * Cwf, deep, gap.reshape(B, cp)


def sspp_reference(ref, knots, ctrl, W, dof=7):
    """The composed SamplingPathPlanner reference of `ctrl` [B, n, dof] on a capsule scene:
    dict(feas, arc, hit [B, npairs], near [B], pairs, feas_nocap).  Feasible = the oracle's
    feasibility without the capsules AND no capsule-pair contact at any waypoint u = i / W; a
    candidate with a capsule distance within 1e-9 of its margin is `near` (left out of parity)."""
    ocap = O.Scene(ref, 0, dof, skip_types=(CAPSULE,))
    movers = {b for b in range(len(ref["body_parent"])) if 0 <= ref["body_qpos_adr"][b] < dof}
    pairs = capsule_pairs(ref, movers)
    _, feas_nocap = O.sspp_score(ocap, knots, 3, ctrl, W)
    arc_all, _ = O.sspp_score(None, knots, 3, ctrl, W)
    B = len(ctrl)
    hit = np.zeros((B, len(pairs)), bool)
    near = np.zeros(B, bool)
    live = np.flatnonzero(feas_nocap)  # (a candidate the other geoms stop is infeasible already)
    if len(live) and pairs:
        qs = sspp_waypoints(knots, ctrl[live], W).reshape(-1, dof)
        xp, xm = fk_all(ocap, qs)
        for k, ((g1, g2, mg), (nc, nd, d, cd)) in enumerate(zip(pairs, pair_results(ref, pairs, xp, xm))):
            hit[live, k] = (nc > 0).reshape(len(live), W + 1).any(1)
            near[live] |= (np.nanmin(np.abs(d - mg), 1) < 1e-9).reshape(len(live), W + 1).any(1)
    feas = (feas_nocap.astype(bool) & ~hit.any(1)).astype(np.uint8)
    arc = np.where(feas == 1, arc_all, np.inf)
    return dict(feas=feas, arc=arc, hit=hit, near=near, pairs=pairs, feas_nocap=feas_nocap)


def pair_types(ref, pairs):
    return [(int(ref["geom_type"][a]), int(ref["geom_type"][b])) for a, b, _ in pairs]


def deciding_types(ref, r):
    """The capsule pair types that alone decide some candidate: infeasible, and feasible without
    that type's pairs.  {type: number of such candidates}."""
    types = pair_types(ref, r["pairs"])
    out = {}
    for t in set(types):
        mine = np.array([x == t for x in types])
        out[t] = int((r["feas_nocap"].astype(bool) & r["hit"][:, mine].any(1) & ~r["hit"][:, ~mine].any(1)).sum())
    return out
