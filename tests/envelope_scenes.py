"""Boundary poses at the edges of the FP32 filter's certified envelope — TEST INFRASTRUCTURE ONLY
(numpy + the CPU oracle; tests/test_envelope_scenes.py checks this module from the reference
alone, tests/test_gpu_filter_envelope.py consumes it).

f32_eps (sspp_kern.h) certifies the filter for root coordinates |x| <= 8 m, partners
within 16 m, pair extents S = r_geom + r_other + margin + |geom offset from its root| <= 8 m with
eps = 2e-4 max(1, S), and at most 64 pairs.  tests/boundary_poses.py puts poses at a threshold in
one corner of that (S = 1, a mover geom at its root, everything within 5 m); the scenes here take
the same machinery (its cases, bisection and poses, through the hooks it documents) to the rest:

  far_in / far_out    the small box mover touching an upright box, a tilted box and a tilted plane
                      (its origin 15 m away) with every root coordinate at 7.5 .. 7.99 m; the same
                      shifted so that the touching root lies at 8.01 .. 8.5 m, where the kernel
                      hands every pair of the waypoint to FP64
  far_partner (_out)  a wall box centred at x = 15.5 m with a half extent of 7.6 m, touched at
                      x = 7.9 m: partner offset, extent and root position near their limits
                      together; the twin's centre lies past 16 m (filter off)
  large2 / 4 / 7      a mover box of 1 m half extents on statics with half extents of metres:
                      S = 2.0, 4.0, 7.5; large_over: S just past 8 (filter off)
  offset_one          one mover geom 1.5 m off the root with a generic local quaternion (the
                      one-geom scan with a relative rotation)
  offset_two          the same and a second offset geom (the per-pair geom reload and its lazy rotation)
  movers              D = 9, two movers of one box each, the second's offset and rotated: the
                      mover-mover pair, the first mover on a static and the second (x, y only) on one

Every case appears at six quaternions (identity, a yaw, both generic ones, one tilted by 1e-6, one
scaled to |q|^2 = 0.3), every scene at the margins 0 and 1e-2.  The offsets from the touching
parameter are relative to the scene table's eps, +-eps {1e-3, 0.1, 0.5, 0.9, 1.1, 2, 4} (for a
table past a cut-off: the eps it would have had), and +-{1e-9, 1e-7} m.
"""
import numpy as np

from tests import boundary_poses as BP
from tests import synth_scenes as Y

MARGINS = (0.0, 1e-2)
EPS_PER_METRE = 2e-4
EPS_FACTORS = (1e-3, 0.1, 0.5, 0.9, 1.1, 2.0, 4.0)
ABS_OFFSETS = (1e-9, 1e-7)

UP = (0.0, 0.0, 1.0)
LAT = (0.011, 0.007, 0.0)
BIG_MOVER = (1.0, 0.8, 0.6)
NUB = (0.4, 0.3, 0.3)
SLAB = (2.4, 0.8, 0.3)
QUATS = ((BP.IDENT, "a"), (BP.q_yaw(BP.YAWS[0]), "b"), (BP.GENERIC[0], "c"), (BP.GENERIC[1], "c"),
         (BP.tilted(BP.IDENT, 1e-6), "d"), (BP.scaled(BP.GENERIC[1], 0.3), "e"))

# the tilted plane of the far scenes: a generic normal, touched near a corner of the cube, its origin 15 m
# away within the plane
PLANE_N = np.array([-0.3, 0.5, 0.8]) / np.linalg.norm([-0.3, 0.5, 0.8])
PLANE_ALONG = np.array([0.5, 0.3, 0.0]) / np.linalg.norm([0.5, 0.3, 0.0])
assert abs(PLANE_N @ PLANE_ALONG) < 1e-15

# the offset geoms of the offset scenes (|pos| = 1.5 and 1.3 m) and the second mover's geom
GEOM_A = dict(pos=(0.9, -0.8, 0.9), quat=tuple(BP.qnorm((0.6, 0.3, -0.5, 0.55))))
GEOM_B = dict(pos=(-0.7, 0.9, -0.6), quat=tuple(BP.qnorm((0.4, -0.6, 0.3, 0.62))))
M1_POS, M1_QUAT = (1.0, 0.5, 3.0), (0.9, 0.1, -0.2, 0.3)
M1_GEOM = dict(size=(0.05, 0.04, 0.03), pos=(0.3, -0.2, 0.25), quat=tuple(BP.qnorm((0.8, -0.3, 0.4, 0.2))))
M1_ARM = BP.rot(M1_QUAT) @ np.array(M1_GEOM["pos"])   # root -> geom centre in the world (fixed rotation)
M0_PARK = (0.0, 0.0, 6.0)
POST = (0.06, 0.05, 0.2)


def _sign_shift(p, by):
    return tuple(x + by * np.sign(x) for x in p)


def _far_statics(out):
    by = 0.4 if out else 0.0
    at = np.array(_sign_shift((7.7, -7.75, -7.7), by))
    return [Y.geom(BP.BOX, BP.BOX_UP, _sign_shift((7.75, 7.7, 7.6), by), name="box_up"),
            Y.geom(BP.BOX, BP.BOX_TILT, _sign_shift((-7.72, 7.7, -7.85), by), BP.QT_BOX, name="box_tilt"),
            Y.geom(BP.PLANE, (0, 0, 1), at - 15.0 * PLANE_ALONG, BP.q_from_to(UP, PLANE_N), name="tplane")], at


def _mover(geoms, name="mover", pos=M0_PARK, quat=(1.0, 0.0, 0.0, 0.0)):
    return Y.body(name, pos, geoms, quat)


def _small(margin, **kw):
    return Y.geom(BP.BOX, Y.MOVER_BOX, name="m_geom", margin=margin, **kw)


def scene(name, margin):
    """(statics, bodies) of one scene."""
    if name in ("far_in", "far_out"):
        return _far_statics(name == "far_out")[0], [_mover([_small(margin)])]
    if name in ("far_partner", "far_partner_out"):
        cx, hx = (15.5, 7.6) if name == "far_partner" else (16.1, 7.7)
        return [Y.geom(BP.BOX, (hx, 0.5, 0.4), (cx, 0.3, -0.2), name="wall"),
                Y.geom(BP.BOX, BP.BOX_UP, (-3.0, -3.0, 2.0), name="box_up")], [_mover([_small(margin)])]
    if name.startswith("large"):
        big = [_mover([Y.geom(BP.BOX, BIG_MOVER, name="m_geom", margin=margin)], pos=(0.0, 0.0, 7.5))]
        slab = Y.geom(BP.BOX, SLAB, (0.0, -4.0, 4.0), BP.QT_BOX, name="slab")
        if name == "large2":
            return [Y.ramp(), Y.geom(BP.BOX, NUB, (0.0, 0.0, 3.0), name="nub")], big
        if name == "large4":
            return [Y.ramp(), slab, Y.geom(BP.BOX, NUB, (0.0, 4.0, 3.0), name="nub")], big
        hx = 6.0 if name == "large7" else 6.6
        return [slab, Y.geom(BP.BOX, (hx, 0.6, 0.4), (0.0, 5.0, 3.0), name="wall")], big
    if name in ("offset_one", "offset_two"):
        st = [Y.ramp(), Y.geom(BP.BOX, BP.BOX_UP, (-4.0, 0.0, 4.0), name="box_up"),
              Y.geom(BP.BOX, BP.BOX_TILT, (4.0, 0.0, 4.0), BP.QT_BOX, name="box_tilt")]
        geoms = [_small(margin, **GEOM_A)]
        if name == "offset_two":
            geoms.append(Y.geom(BP.BOX, Y.MOVER_BOX, name="m_geom2", margin=margin, **GEOM_B))
        return st, [_mover(geoms, pos=(0.0, 0.0, 7.0))]
    if name == "movers":
        st = [Y.geom(BP.BOX, BP.BOX_UP, (-3.0, -2.0, 2.0), name="box_up"),
              Y.geom(BP.BOX, POST, (4.0, -3.0, M1_POS[2] + M1_ARM[2]), name="post")]
        m1 = Y.geom(BP.BOX, M1_GEOM["size"], M1_GEOM["pos"], M1_GEOM["quat"], name="b_box", margin=margin)
        return st, [_mover([_small(margin)], "m0"), _mover([m1], "m1", M1_POS, M1_QUAT)]
    raise ValueError(name)


SCENES = ("far_in", "far_out", "far_partner", "far_partner_out", "large2", "large4", "large7", "large_over",
          "offset_one", "offset_two", "movers")
DOF = {name: 9 if name == "movers" else 7 for name in SCENES}
# what config()["scan"] must say of a full-table launch with the filter asked for
SCAN = {name: "fp64" if name in ("far_partner_out", "large_over") else "fp32-filtered" for name in SCENES}
# |root coordinate| of every pose, on every axis: (least, most)
ROOT_RANGE = {"far_in": (7.5, 7.99), "far_out": (8.01, 8.5)}


def _families(make):
    return [make(q, f) for q, f in QUATS]


def _arm(g):
    """root -> geom centre in the world, of a mover geom at g["pos"] and the root's quaternion."""
    pos = np.array(g["pos"])
    return lambda q: BP.rot(q) @ pos


def cases(name):
    """The cases of one scene (each a boundary_poses case, some with its hooks set)."""
    bb, pb = "box-box", "plane-box"
    cs = []
    if name in ("far_in", "far_out"):
        at = _far_statics(name == "far_out")[1]
        cs += _families(lambda q, f: BP._case(bb, "upright", "box_up", q, UP, LAT, family=f))
        cs += _families(lambda q, f: BP._case(bb, "tilted", "box_tilt", q, UP, LAT, family=f))
        cs += _families(lambda q, f: dict(BP._case(pb, "tilted far origin", "tplane", q, PLANE_N + 0.2 * PLANE_ALONG,
                                                   family=f), origin=at))
    elif name in ("far_partner", "far_partner_out"):
        hx = 7.6 if name == "far_partner" else 7.7
        cs += _families(lambda q, f: BP._case(bb, "wall end", "wall", q, (-1.0, 0.0, 0.0), (-hx + 0.05, 0.011, 0.007), family=f))
        cs += _families(lambda q, f: BP._case(bb, "wall end oblique", "wall", q, (-1.0, 0.3, 0.2), (-hx + 0.05, 0.0, 0.0), family=f))
        cs += _families(lambda q, f: BP._case(bb, "upright", "box_up", q, UP, LAT, family=f))
    elif name.startswith("large"):
        far = dict(t_clear=4.0)
        if name in ("large2", "large4"):
            cs += _families(lambda q, f: dict(BP._case(bb, "nub top", "nub", q, UP, LAT, family=f), **far))
            cs += _families(lambda q, f: dict(BP._case(bb, "nub oblique", "nub", q, (0.3, -0.2, 1.0), family=f), **far))
            # the ramp passes 0.558 m above its origin's height at y = 3
            cs += _families(lambda q, f: dict(BP._case(pb, "ramp", "ramp", q, (0.0, 0.3, 1.0), (-5.0, 3.0, 0.6), family=f), **far))
        if name != "large2":
            cs += _families(lambda q, f: dict(BP._case(bb, "slab end", "slab", q, UP, (2.0, 0.5, 0.0), frame="target", family=f), **far))
            cs += _families(lambda q, f: dict(BP._case(bb, "slab oblique", "slab", q, (0.3, -0.2, 1.0), family=f), **far))
        if name in ("large7", "large_over"):
            hx = 6.0 if name == "large7" else 6.6
            cs += _families(lambda q, f: dict(BP._case(bb, "wall side", "wall", q, (0.0, -1.0, 0.0), (5.5, -0.5, 0.05), family=f), **far))
            cs += _families(lambda q, f: dict(BP._case(bb, "wall top", "wall", q, UP, (-5.5, 0.1, 0.0), family=f), **far))
            cs += _families(lambda q, f: dict(BP._case(bb, "wall end", "wall", q, (1.0, 0.1, 0.05), (hx - 0.1, 0.0, 0.0), family=f), **far))
    elif name in ("offset_one", "offset_two"):
        for tag, g in (("", GEOM_A),) + ((("2", GEOM_B),) if name == "offset_two" else ()):
            arm = dict(offset=_arm(g), geom="m_geom" + tag)
            cs += _families(lambda q, f: dict(BP._case(bb, "upright" + tag, "box_up", q, UP, LAT, family=f), **arm))
            cs += _families(lambda q, f: dict(BP._case(bb, "tilted" + tag, "box_tilt", q, (0.3, -0.2, 1.0), (0.01, 0.0, 0.0), family=f), **arm))
        if name == "offset_one":
            # a point of the ramp 5 m from its origin: (0, -5, -0.05 - 5 tan 0.2)
            n = BP.rot(Y.RAMP_QUAT)[:, 2]
            at = np.array(Y.RAMP_POS) + np.array([0.0, -5.0, 5.0 * n[1] / n[2]])
            cs += _families(lambda q, f: dict(BP._case(pb, "ramp", "ramp", q, (0.0, 0.3, 1.0), family=f), origin=at,
                                              offset=_arm(GEOM_A), geom="m_geom"))
    elif name == "movers":
        m1_xy = M1_POS[:2]
        row0 = lambda p, q: np.concatenate([p, q, m1_xy])                 # noqa: E731  (mover 0 moves)
        row1 = lambda p, q: np.concatenate([M0_PARK, q, p[:2]])           # noqa: E731  (mover 1 moves, in x and y)
        b_box = np.array(M1_POS) + M1_ARM
        cs += _families(lambda q, f: dict(BP._case(bb, "mover-mover", "b_box", q, UP, (0.004, 0.003, 0.0), family=f),
                                          origin=b_box, pose=row0, geom="m_geom"))
        cs += _families(lambda q, f: dict(BP._case(bb, "mover-mover oblique", "b_box", q, (0.3, -0.2, 1.0), family=f),
                                          origin=b_box, pose=row0, geom="m_geom"))
        cs += _families(lambda q, f: dict(BP._case(bb, "first on static", "box_up", q, UP, LAT, family=f), pose=row0,
                                          geom="m_geom"))
        cs += _families(lambda q, f: dict(BP._case(bb, "second on static", "post", q, (-1.0, 0.3, 0.0), (0.01, 0.005, 0.0),
                                                   family=f), pose=row1, offset=lambda _q: M1_ARM, geom="b_box"))
    else:
        raise ValueError(name)
    return cs


# ------------------------------------------------------------------ the table's eps
def table_extent(ref, dof):
    """S of a scene's full pair table by f32_eps's formula, cut-offs aside: the largest
    r_geom + r_other + margin + |moving geom's offset from its root| (at least 1)."""
    S = 1.0
    for gm, go in Y.moving_pairs(ref, dof):
        S = max(S, Y._rbound(ref["geom_type"][gm], ref["geom_size"][gm]) + Y._rbound(ref["geom_type"][go], ref["geom_size"][go]) +
                max(ref["geom_margin"][gm], ref["geom_margin"][go]) + float(np.linalg.norm(ref["geom_pos"][gm])))
    return S


def offsets(eps):
    mags = [eps * f for f in EPS_FACTORS] + list(ABS_OFFSETS)
    return tuple(s * m for m in mags for s in (-1.0, 1.0))


_MEMO = {}


def envelope_set(root, name, margin):
    """(ref, cases, poses, eps) of one scene and margin, once per process."""
    key = (name, margin)
    if key not in _MEMO:
        _, ref_path = BP.write_scene(root, "env_%s_m%g" % (name, margin), scene(name, margin))
        ref = BP.Ref(ref_path, 0, DOF[name])
        eps = EPS_PER_METRE * table_extent(ref.ref, DOF[name])
        cs = [dict(c, offsets=offsets(eps)) for c in cases(name)]
        _MEMO[key] = (ref, cs, BP.poses_of(ref, cs), eps)
    return _MEMO[key]

