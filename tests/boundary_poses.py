"""Boundary poses: mover configurations a known distance from a contact threshold — TEST
INFRASTRUCTURE ONLY (numpy + the CPU oracle; tests/test_boundary_poses.py checks this module,
tests/test_gpu_boundary_poses.py and the host narrowphase check consume it).

A case fixes a pair type, a contact feature, the mover's quaternion and a unit approach direction
d pointing away from the target static.  The mover's root moves on the line anchor + t d: at
t = 0 it certainly overlaps the target, at t = T_CLEAR it is certainly clear.  The touching
parameter touch(d) is bisected (60 steps) on the reference's decision — oracle.Scene.contacts, or
for the scenes with a capsule in them the composed reference of tests/capsule_scenes.py (the
oracle without the capsules + tests/capsule_ref.py on the capsule pairs).  Both bodies are convex
and every rule's decision quantity is convex in t (a distance, the maximum of SAT separations,
the bounding-sphere distance), so the decision changes once on the line.  The poses of a case are
anchor + (touch + off) d for every off in OFFSETS: contact (or deep contact) exactly for off < 0;
two more poses sit at the bisection's own ends, a rounding step apart (ENDS).

Thresholds: the contact threshold dist < margin at the margins MARGINS (the mover geom carries
the margin: one scene per margin), and for the TaskSpacePlanner scenes the deep threshold
dist < -1e-3, bisected on the reference's deep count.

Orientation families of the mover's quaternion: (a) identity, (b) yaw only (exactly upright),
(c) generic unit quaternions, (d) a member of (a) / (b) turned by THETAS about the world x axis
(box-box edge axes on both sides of the FP64 cut |L| = 1e-6, upright3 / cyl_vertical just off),
(e) a quaternion scaled to |q|^2 = 0.2 or 0.3 (unnormalised control rows: the FP32 filter hands
quaternions shorter than 0.25 to FP64).

A sphere whose centre lies inside a box has dist <= -r: with the scenes' radii that is far
below every threshold, so the sphere-box cases stop at the face, edge and corner regions; the
centre-inside rule is covered away from a threshold (SPHERE_INSIDE, used by the host check).
"""
import os

import numpy as np

from oracle import mjcf_ref
from oracle import oracle as O
from tests import capsule_ref as R
from tests import capsule_scenes as CS
from tests import synth_scenes as Y

PLANE, SPHERE, CAPSULE, CYLINDER, BOX = 0, 2, 3, 5, 6
TYPE_NAMES = {PLANE: "plane", SPHERE: "sphere", CAPSULE: "capsule", CYLINDER: "cylinder", BOX: "box"}

_MAGS = (1e-12, 1e-9, 1e-7, 1e-6, 1e-5, 5e-5, 1e-4, 2e-4, 3e-4, 1e-3)
OFFSETS = tuple(s * m for m in _MAGS for s in (-1.0, 1.0))
# and the bisection's own ends, as off = -0.0 (the last touching parameter) and +0.0 (the first
# clear one, one rounding step on): the reference's decision there is known by construction.
# Only for the pair types the CPU oracle decides: it restates the device code operation by
# operation, while tests/capsule_ref.py (numpy) promises the capsule distances to 1e-12, not to
# the last bit.  And only for the SamplingPathPlanner sets, whose control rows reach the kernels
# as given: a TaskSpacePlanner candidate's waypoints come from a spline interpolated through its
# vias, the pose within a few ulp on either side.
ENDS = (-0.0, 0.0)


def offsets_of(c):
    if "offsets" in c:   # a scene's own offsets (tests/envelope_scenes.py: relative to its table's eps)
        return c["offsets"]
    return OFFSETS if "capsule" in c["pair"] or "yaw" in c else OFFSETS + ENDS
MARGINS = (0.0, 1e-3, 1e-2)
THETAS = (5e-7, 1e-6, 2e-6, 1e-5, 3e-5)
DEEP = -1e-3
FLOOR = 1e-9      # the least |off| at which the decision must follow the sign of off
FLOORS = {}       # pair type -> a measured floor above FLOOR (none: every type meets 1e-9)
T_CLEAR = 1.0     # the far end of every approach line (statics are 2.5 m apart)
N_BISECT = 60

# table sizes: the scene's own pairs (fewer than 9), 12 (the survivors' hull masks on) and 65
# (the FP32 filter off, test_gpu_synthetic_scenes.GRIDS' (5, 13))
TABLES = {"small": None, "hull": 12, "big": 65}
FILLER_BOX = (0.02, 0.025, 0.03)   # synth_scenes.grid's static boxes

MOVER_GEOMS = {"box": (BOX, Y.MOVER_BOX), "sphere": (SPHERE, (0.03,)), "cylinder": (CYLINDER, (0.025, 0.04)),
               "capsule": (CAPSULE, (0.025, 0.05)), "boxcap": (BOX, Y.MOVER_BOX)}
Z_STATICS = 2.0
SLOTS = [(x, y, Z_STATICS) for y in (-2.5, 2.5) for x in (-5.0, -2.5, 0.0, 2.5, 5.0)]
BOX_UP = (0.1, 0.08, 0.06)
BOX_TILT = (0.06, 0.1, 0.04)
QT_BOX = (0.8, 0.1, 0.5, 0.3)
QT_CYL = (0.92, 0.3, 0.2, 0.1)


# ------------------------------------------------------------------ quaternions
def qnorm(q):
    q = np.asarray(q, float)
    return q / np.linalg.norm(q)


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def q_axis(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * axis])


def q_yaw(yaw):
    """Exactly (w, 0, 0, z): the rotation matrix keeps its exact zeros."""
    return np.array([np.cos(0.5 * yaw), 0.0, 0.0, np.sin(0.5 * yaw)])


def q_from_to(a, b):
    """The shortest rotation taking the direction a to the direction b (not opposite)."""
    a, b = np.asarray(a, float) / np.linalg.norm(a), np.asarray(b, float) / np.linalg.norm(b)
    return qnorm(np.concatenate([[1.0 + a @ b], np.cross(a, b)]))


def rot(q):
    return CS.quat2mat(q).reshape(3, 3)


IDENT = np.array([1.0, 0.0, 0.0, 0.0])
# about y: BOX_TILT's diagonal (e0, 0, e2) to +z, so one of its edges along y is its highest feature
EDGE_UP = tuple(q_from_to((BOX_TILT[0], 0.0, BOX_TILT[2]), (0.0, 0.0, 1.0)))
YAWS = (0.3, np.pi / 2)
GENERIC = (qnorm((0.7, -0.2, 0.5, 0.4)), qnorm((0.3, 0.6, -0.1, 0.7)))
X_AXIS = (1.0, 0.0, 0.0)


def tilted(q, theta):
    """q turned by theta about the world x axis (family d)."""
    return qmul(q_axis(X_AXIS, theta), q)


def scaled(q, n2):
    """q scaled to |q|^2 = n2 (family e)."""
    return qnorm(q) * np.sqrt(n2)


def family_of(q):
    q = np.asarray(q, float)
    if abs(q @ q - 1.0) > 1e-3:
        return "e"
    if np.array_equal(q, IDENT):
        return "a"
    if q[1] == 0.0 and q[2] == 0.0:
        return "b"
    return "c"


# ------------------------------------------------------------------ scenes
def _statics(kind):
    """The target statics of one mover kind: name -> geom, each on its own slot."""
    box_up = Y.geom(BOX, BOX_UP, name="box_up")
    box_tilt = Y.geom(BOX, BOX_TILT, quat=QT_BOX, name="box_tilt")
    ball = Y.geom(SPHERE, 0.08, name="ball")
    if kind == "box":
        st = [ball, Y.geom(CYLINDER, (0.05, 0.12), name="cyl_up"),
              Y.geom(CYLINDER, (0.04, 0.15), quat=QT_CYL, name="cyl_tilt"), box_up,
              Y.geom(BOX, BOX_TILT, quat=EDGE_UP, name="box_edge"), box_tilt,
              Y.geom(BOX, BOX_UP, quat=tuple(q_yaw(0.7)), name="box_yaw")]
    elif kind == "sphere":
        st = [ball, Y.geom(CYLINDER, (0.04, 0.15), quat=QT_CYL, name="cyl_tilt"), box_tilt,
              CS.capsule(0.03, 0.1, quat=QT_CYL, name="cap_tilt")]
    elif kind == "cylinder":
        st = [ball, box_up, box_tilt]
    elif kind == "capsule":
        st = [ball, CS.capsule(0.03, 0.1, name="cap_up"), CS.capsule(0.03, 0.1, quat=QT_CYL, name="cap_tilt"),
              box_up, box_tilt]
    elif kind == "boxcap":
        st = [CS.capsule(0.03, 0.1, name="cap_up"), CS.capsule(0.03, 0.1, quat=QT_CYL, name="cap_tilt")]
    else:
        raise ValueError(kind)
    return [dict(g, pos=SLOTS[i]) for i, g in enumerate(st)]


def _fillers(n):
    """n far-away static boxes at general rotations that no pose of a case comes near."""
    rng = np.random.default_rng(4242)
    out = []
    for k in range(n):
        q = rng.normal(size=4)
        out.append(Y.geom(BOX, FILLER_BOX, (-6.0 + 0.2 * k, 6.5 + 0.3 * (k % 3), 4.0 + 0.25 * (k % 4)), q / np.linalg.norm(q),
                          name="fill%02d" % k))
    return out


def _mover(kind, margin):
    t, size = MOVER_GEOMS[kind]
    return Y.body("mover", (0.0, 0.0, 6.0), [Y.geom(t, size, name="m_geom", margin=margin)])


def sspp_scene(kind, margin, table):
    """(statics, bodies) of the SamplingPathPlanner scene of one mover kind, margin and table size."""
    st = ([Y.ramp()] if kind != "boxcap" else []) + _statics(kind)
    want = TABLES[table]
    if want is not None:
        st = st + _fillers(want - len(st))
    return st, [_mover(kind, margin)]


def tsp_scene(name):
    """The TaskSpacePlanner scenes (yaw-only box mover): "up" every static box upright (the UP
    kernels), "cb2" vertical cylinders and upright boxes only (CB = 2), "generic" the same with
    one tilted box and one tilted cylinder, "capsule" a vertical and a tilted capsule."""
    floor = Y.geom(PLANE, (0, 0, 1), name="floor")
    box_up = Y.geom(BOX, BOX_UP, name="box_up")
    box_yaw = Y.geom(BOX, BOX_UP, quat=tuple(q_yaw(0.7)), name="box_yaw")
    cyl_up = Y.geom(CYLINDER, (0.05, 0.12), name="cyl_up")
    if name == "up":
        st = [box_up, box_yaw]
    elif name == "cb2":
        st = [box_up, cyl_up, Y.geom(CYLINDER, (0.06, 0.08), name="cyl_up2")]
    elif name == "generic":
        st = [box_up, cyl_up, Y.geom(BOX, BOX_TILT, quat=QT_BOX, name="box_tilt"),
              Y.geom(CYLINDER, (0.04, 0.15), quat=QT_CYL, name="cyl_tilt"), Y.geom(SPHERE, 0.08, name="ball")]
    elif name == "capsule":
        st = [box_up, CS.capsule(0.03, 0.1, name="cap_up"), CS.capsule(0.03, 0.1, quat=QT_CYL, name="cap_tilt")]
    else:
        raise ValueError(name)
    st = [floor] + [dict(g, pos=SLOTS[i]) for i, g in enumerate(st)]
    return st, [Y.body("mover", (0.0, 0.0, 6.0), [Y.geom(BOX, Y.MOVER_BOX, name="m_geom")])]


TSP_SCENES = ("up", "cb2", "generic", "capsule")


# ------------------------------------------------------------------ the reference's decision
class Ref:
    """One scene on the reference side: contacts(q) -> (contact count, deep count) of the moving
    pairs, composed with tests/capsule_ref.py where the scene holds capsules."""

    def __init__(self, path, mode, arg):
        self.ref = mjcf_ref.load(path)
        if isinstance(arg, str):
            arg = self.ref["body_names"].index(arg)
        self.mode, self.arg = mode, arg
        self.has_capsule = bool((np.asarray(self.ref["geom_type"]) == CAPSULE).any())
        self.oscene = O.Scene(self.ref, mode, arg, skip_types=(CAPSULE,) if self.has_capsule else ())
        self.full = O.Scene(self.ref, mode, arg)   # pair counts and forward kinematics (type-blind)
        if mode == 0:
            movers = {b for b in range(len(self.ref["body_parent"])) if 0 <= self.ref["body_qpos_adr"][b] < arg}
        else:
            movers = {arg}
        self.cap_pairs = CS.capsule_pairs(self.ref, movers) if self.has_capsule else []
        self.names = list(self.ref["geom_names"])

    def geom(self, name):
        return self.names.index(name)

    def contacts(self, q):
        n, _, nd = self.oscene.contacts(q)
        if self.cap_pairs:
            xp, xm = self.oscene.fk(q)
            gt, gs = self.ref["geom_type"], np.asarray(self.ref["geom_size"], float)
            for g1, g2, mg in self.cap_pairs:
                thr = R_bound(gt[g1], gs[g1]) + R_bound(gt[g2], gs[g2]) + mg
                dc = xp[g2] - xp[g1]
                if gt[g1] != PLANE and dc @ dc > thr * thr:
                    continue   # the bounding-sphere cull every pair passes first
                nc, ndp, _ = R.collide(gt[g1], xp[g1], xm[g1], gs[g1], gt[g2], xp[g2], xm[g2], gs[g2], mg)
                n += int(nc[0])
                nd += int(ndp[0])
        return n, nd


def R_bound(t, s):
    """sspd::geom_rbound."""
    if t == BOX:
        return float(np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]))
    if t == CYLINDER:
        return float(np.sqrt(s[0] * s[0] + s[1] * s[1]))
    if t == SPHERE:
        return float(s[0])
    if t == CAPSULE:
        return float(s[0] + s[1])
    return 0.0


# ------------------------------------------------------------------ cases
def _case(pair, feature, target, quat, d, anchor=(0.0, 0.0, 0.0), frame="world", family=None, closed=None):
    """anchor and d in the world's axes or in the target's (frame="target"), anchor relative to
    the target's centre.  closed: the touching parameter's closed form, a function of (margin,
    the case's world direction, the reference) or None."""
    quat = np.asarray(quat, float)
    return dict(pair=pair, feature=feature, target=target, quat=quat, d=np.asarray(d, float) / np.linalg.norm(d),
                anchor=np.asarray(anchor, float), frame=frame, family=family or family_of(quat), closed=closed)


def _with_families(make, bases=(IDENT,) + tuple(q_yaw(y) for y in YAWS), generic=GENERIC, thetas=THETAS,
                   tilt_of=(IDENT, q_yaw(YAWS[0])), scale_of=None):
    """make(quat, family) for the families a, b (bases), c (generic), d (tilt_of x thetas), e."""
    out = [make(q, None) for q in bases] + [make(q, "c") for q in generic]
    out += [make(tilted(q, th), "d") for q in tilt_of for th in thetas]
    scale_of = generic[:1] + (q_yaw(YAWS[0]),) if scale_of is None else scale_of
    out += [make(scaled(q, n2), "e") for q, n2 in zip(scale_of, (0.2, 0.3))]
    return out


def _plane_closed(kind):
    size = MOVER_GEOMS[kind][1]

    def f(margin, c, ref):
        n = ref_mat(ref, "ramp")[:, 2]
        if kind == "sphere":
            reach = size[0]
        else:
            A = rot(c["quat"])
            reach = sum(abs(n @ A[:, j]) * size[j] for j in range(3))
        return (reach + margin) / (c["d_world"] @ n)
    return f


def ref_mat(ref, name):
    g = ref.geom(name)
    return CS.quat2mat(ref.ref["geom_quat"][g]).reshape(3, 3)


def sspp_cases(kind):
    """The cases of one SamplingPathPlanner scene."""
    up = (0.0, 0.0, 1.0)
    lat = (0.011, 0.007, 0.0)
    diag_xz = (1.0, 0.0, 1.0)
    cs = []
    if kind in ("box", "boxcap"):
        e = np.array(Y.MOVER_BOX)
        ediag = (e[0], 0.0, e[2])
    if kind == "box":
        pb = "plane-box"
        cs += _with_families(lambda q, f: _case(pb, "corner", "ramp", q, (0.0, 0.3, 1.0), family=f, closed=_plane_closed("box")))
        sb = "sphere-box"
        cs += _with_families(lambda q, f: _case(sb, "face", "ball", q, up, lat, family=f,
                                                closed=(lambda m, c, r: 0.08 + e[2] + m) if f in (None,) else None),
                             generic=GENERIC[:1], tilt_of=(IDENT,))
        # the mover box's edge / corner towards the ball: the ball's centre leaves the box through them
        cs += [_case(sb, "edge", "ball", q, (0.0, e[1], e[2]), (0.0, 0.2 * e[1], 0.2 * e[2])) for q in (IDENT,)]
        cs += [_case(sb, "edge", "ball", q_yaw(np.pi / 2), (0.0, e[0], e[2]), (0.0, 0.2 * e[0], 0.2 * e[2]))]
        cs += [_case(sb, "corner", "ball", IDENT, e, 0.2 * e)]
        cb = "cylinder-box"
        cs += _with_families(lambda q, f: _case(cb, "cap-face upright", "cyl_up", q, up, lat, family=f), generic=GENERIC[:1])
        cs += [_case(cb, "cap-face", "cyl_tilt", qnorm(QT_CYL), up, lat, frame="target"),
               # the mover's edge along y leads along (e0, 0, e2): towards the rim as the box stands,
               # towards the side when that diagonal is turned (about y) into the radial direction
               _case(cb, "rim-edge upright", "cyl_up", IDENT, ediag, (0.03, 0.0, 0.1)),
               _case(cb, "rim-edge", "cyl_tilt", qnorm(QT_CYL), ediag, (0.02, 0.0, 0.13), frame="target"),
               _case(cb, "side-edge", "cyl_up", q_from_to(ediag, X_AXIS), X_AXIS, (0.0, 0.0, 0.01)),
               _case(cb, "side-edge", "cyl_tilt", qmul(qnorm(QT_CYL), q_from_to(ediag, X_AXIS)), X_AXIS, (0.0, 0.0, 0.01),
                     frame="target"),
               _case(cb, "side-face", "cyl_tilt", GENERIC[1], (0.2, 1.0, 0.1))]
        bb = "box-box"
        cs += _with_families(lambda q, f: _case(bb, "face-face", "box_up", q, up, lat, family=f,
                                                closed=(lambda m, c, r: BOX_UP[2] + e[2] + m) if f is None else None),
                             tilt_of=(IDENT, q_yaw(YAWS[0]), q_yaw(YAWS[1])))
        cs += [_case(bb, "face-face", "box_yaw", q_yaw(0.7), up, lat, closed=lambda m, c, r: BOX_UP[2] + e[2] + m),
               _case(bb, "face-face", "box_yaw", q_yaw(-0.4), up, lat, closed=lambda m, c, r: BOX_UP[2] + e[2] + m)]
        cs += [_case(bb, "face-face", "box_yaw", tilted(q_yaw(0.7), th), up, lat, family="d") for th in THETAS]
        # the mover's edge along x straight down, over box_edge's edge along y straight up
        x_down = q_from_to((0.0, e[1], e[2]), (0.0, 0.0, -1.0))
        cs += [_case(bb, "edge-edge", "box_edge", x_down, up, (0.0, 0.0, 0.0)),
               _case(bb, "edge-edge", "box_edge", qmul(q_yaw(0.2), x_down), up, (0.004, 0.003, 0.0))]
        cs += [_case(bb, "edge-edge", "box_edge", tilted(x_down, th), up, family="d") for th in THETAS[:2]]
        down = q_from_to(e, (0.0, 0.0, -1.0))          # a corner of the mover straight down
        cs += [_case(bb, "corner-face", "box_up", down, up, lat),
               _case(bb, "corner-face", "box_tilt", qmul(qnorm(QT_BOX), down), up, (0.01, 0.006, 0.0), frame="target")]
        u = np.array(BOX_UP) / np.linalg.norm(BOX_UP)
        cs += [_case(bb, "corner-corner", "box_up", q_from_to(e, u), u),
               _case(bb, "corner-corner", "box_tilt", qmul(qnorm(QT_BOX), q_from_to(e, np.array(BOX_TILT))),
                     np.array(BOX_TILT), frame="target")]
        cs += [_case(bb, "generic", "box_tilt", q, dd, a) for q, dd, a in
               ((GENERIC[0], (0.3, -0.2, 1.0), (0.01, 0.0, 0.0)), (GENERIC[1], (-1.0, 0.4, 0.2), (0.0, 0.01, 0.0)),
                (IDENT, (0.1, 1.0, 0.3), (0.0, 0.0, 0.01)), (q_yaw(YAWS[0]), (1.0, 0.2, -0.1), (0.0, 0.0, 0.0)))]
        cs += [_case(bb, "generic", "box_tilt", scaled(GENERIC[1], 0.3), (0.3, -0.2, 1.0), family="e")]
    elif kind == "sphere":
        r = MOVER_GEOMS["sphere"][1][0]
        cs += [_case("plane-sphere", "point", "ramp", q, dd, closed=_plane_closed("sphere"))
               for q, dd in ((IDENT, (0.0, 0.0, 1.0)), (q_yaw(0.3), (0.3, 0.3, 1.0)), (GENERIC[0], (0.0, -0.2, 1.0)),
                             (scaled(GENERIC[0], 0.2), (0.1, 0.0, 1.0)))]
        cs += [_case("sphere-sphere", "point", "ball", q, dd, closed=lambda m, c, rf: 0.08 + r + m)
               for q, dd in ((IDENT, X_AXIS), (q_yaw(0.3), (0.3, -0.5, 0.8)), (GENERIC[1], (-0.6, 0.1, 0.2)),
                             (scaled(GENERIC[1], 0.3), (0.0, 1.0, 0.0)))]
        sc = "sphere-cylinder"
        cs += [_case(sc, "cap", "cyl_tilt", IDENT, up, (0.01, 0.005, 0.0), frame="target"),
               _case(sc, "side", "cyl_tilt", q_yaw(0.3), (1.0, 0.3, 0.0), (0.0, 0.0, 0.05), frame="target"),
               _case(sc, "rim", "cyl_tilt", GENERIC[0], diag_xz, (0.03, 0.0, 0.14), frame="target")]
        sb = "sphere-box"
        bt = np.array(BOX_TILT)
        cs += [_case(sb, "face", "box_tilt", IDENT, up, (0.01, 0.02, 0.0), frame="target",
                     closed=lambda m, c, rf: BOX_TILT[2] + r + m),
               _case(sb, "edge", "box_tilt", q_yaw(0.3), (0.0, 1.0, 1.0), (0.01, bt[1] - 0.01, bt[2] - 0.01), frame="target"),
               _case(sb, "corner", "box_tilt", GENERIC[1], (1.0, 1.0, 1.0), bt - 0.01, frame="target"),
               _case(sb, "corner", "box_tilt", scaled(GENERIC[0], 0.2), (1.0, 1.0, 1.0), bt - 0.01, frame="target")]
        cs += [_case("sphere-capsule", "side", "cap_tilt", IDENT, (1.0, 0.2, 0.0), (0.0, 0.0, 0.04), frame="target"),
               _case("sphere-capsule", "end", "cap_tilt", q_yaw(0.3), (0.1, 0.1, 1.0), (0.0, 0.0, 0.09), frame="target")]
    elif kind == "cylinder":
        pc = "plane-cylinder"
        # the ramp's normal is (0, -sin 0.2, cos 0.2): the world x axis lies in the plane exactly
        cs += [_case(pc, "parallel", "ramp", q_from_to(up, X_AXIS), up),
               _case(pc, "perpendicular", "ramp", qnorm(Y.RAMP_QUAT), (0.0, 0.1, 1.0))]
        cs += [_case(pc, "parallel", "ramp", tilted(q_from_to(up, X_AXIS), th) if i % 2 else
                     qmul(q_axis((0.0, 1.0, 0.0), th), q_from_to(up, X_AXIS)), up, family="d") for i, th in enumerate(THETAS)]
        cs += _with_families(lambda q, f: _case(pc, "oblique", "ramp", q, (0.0, 0.2, 1.0), family=f), thetas=THETAS[:2])
        sc = "sphere-cylinder"
        cs += [_case(sc, "cap", "ball", IDENT, up, (0.004, 0.003, 0.0)),
               _case(sc, "side", "ball", q_yaw(0.3), (1.0, 0.3, 0.0), (0.0, 0.0, 0.01)),
               _case(sc, "rim", "ball", GENERIC[0], (0.5, -0.2, 1.0)),
               _case(sc, "rim", "ball", scaled(GENERIC[0], 0.2), (0.5, -0.2, 1.0))]
        cb = "cylinder-box"
        cs += _with_families(lambda q, f: _case(cb, "cap-face upright", "box_up", q, up, lat, family=f), generic=GENERIC[:1])
        to_diag = q_from_to(up, (1.0, 0.0, -1.0))       # the axis across the box's top edge along y
        cs += [_case(cb, "rim-edge upright", "box_up", IDENT, diag_xz, (BOX_UP[0] - 0.01, 0.0, BOX_UP[2] - 0.01)),
               _case(cb, "side-edge", "box_up", to_diag, diag_xz, (BOX_UP[0] - 0.01, 0.0, BOX_UP[2] - 0.01)),
               _case(cb, "cap-face", "box_tilt", qnorm(QT_BOX), up, (0.01, 0.02, 0.0), frame="target"),
               _case(cb, "rim-edge", "box_tilt", qnorm(QT_BOX), diag_xz, (BOX_TILT[0] - 0.01, 0.0, BOX_TILT[2] - 0.01),
                     frame="target"),
               _case(cb, "side-edge", "box_tilt", qmul(qnorm(QT_BOX), to_diag), diag_xz,
                     (BOX_TILT[0] - 0.01, 0.0, BOX_TILT[2] - 0.01), frame="target"),
               _case(cb, "generic", "box_tilt", GENERIC[1], (-0.3, 1.0, 0.2))]
    elif kind == "capsule":
        pc = "plane-capsule"
        lying = q_from_to(up, X_AXIS)
        cs += [_case(pc, "perpendicular", "ramp", qnorm(Y.RAMP_QUAT), (0.0, 0.1, 1.0)),
               _case(pc, "parallel", "ramp", lying, up),
               _case(pc, "oblique", "ramp", IDENT, up), _case(pc, "oblique", "ramp", q_yaw(0.3), (0.2, 0.0, 1.0)),
               _case(pc, "oblique", "ramp", GENERIC[0], up), _case(pc, "oblique", "ramp", scaled(GENERIC[0], 0.2), up)]
        cs += [_case(pc, "parallel", "ramp", qmul(q_axis((0.0, 1.0, 0.0), th), lying), up, family="d") for th in THETAS]
        cs += [_case("sphere-capsule", "side", "ball", IDENT, (1.0, 0.3, 0.0), (0.0, 0.0, 0.01)),
               _case("sphere-capsule", "end", "ball", GENERIC[1], rot(GENERIC[1])[:, 2])]
        cc = "capsule-capsule"
        cs += [_case(cc, "parallel", "cap_up", IDENT, (1.0, 0.2, 0.0), (0.0, 0.0, 0.02)),
               _case(cc, "parallel", "cap_up", q_yaw(0.3), (0.4, -1.0, 0.0), (0.0, 0.0, -0.03)),
               _case(cc, "collinear", "cap_up", IDENT, up),
               _case(cc, "crossing", "cap_up", q_from_to(up, (0.0, 1.0, 0.0)), X_AXIS, (0.0, 0.0, 0.02)),
               _case(cc, "generic", "cap_tilt", GENERIC[0], (0.2, 1.0, 0.4)),
               _case(cc, "generic", "cap_tilt", scaled(GENERIC[1], 0.3), (1.0, -0.2, 0.1))]
        cs += [_case(cc, "parallel", "cap_up", tilted(IDENT, th), (1.0, 0.2, 0.0), (0.0, 0.0, 0.02), family="d") for th in THETAS]
        kb = "capsule-box"
        cs += [_case(kb, "end-face", "box_up", IDENT, up, lat), _case(kb, "end-face", "box_up", q_yaw(0.3), up, lat),
               _case(kb, "side-face", "box_up", lying, up, lat),
               _case(kb, "side-edge", "box_up", q_from_to(up, (1.0, 0.0, -1.0)), diag_xz,
                     (BOX_UP[0] - 0.01, 0.0, BOX_UP[2] - 0.01)),
               _case(kb, "corner", "box_tilt", GENERIC[0], (1.0, 1.0, 1.0), np.array(BOX_TILT) - 0.01, frame="target"),
               _case(kb, "generic", "box_tilt", GENERIC[1], (0.2, -1.0, 0.3))]
        cs += [_case(kb, "side-face", "box_up", qmul(q_axis((0.0, 1.0, 0.0), th), lying), up, lat, family="d") for th in THETAS[:3]]
    elif kind == "boxcap":
        kb = "capsule-box"
        cs += [_case(kb, "end-face", "cap_up", IDENT, up, (0.004, 0.003, 0.0)),
               _case(kb, "side-face", "cap_up", q_yaw(0.3), (1.0, 0.1, 0.0), (0.0, 0.0, 0.02)),
               _case(kb, "side-edge", "cap_up", qmul(q_yaw(np.pi / 4), q_axis(X_AXIS, 0.6)), X_AXIS, (0.0, 0.0, 0.01)),
               _case(kb, "generic", "cap_tilt", GENERIC[0], (0.2, 1.0, 0.4)),
               _case(kb, "generic", "cap_tilt", scaled(GENERIC[1], 0.3), (1.0, -0.2, 0.1))]
        cs += [_case(kb, "end-face", "cap_up", tilted(IDENT, th), up, (0.004, 0.003, 0.0), family="d") for th in THETAS[:3]]
    return cs


SSPP_KINDS = ("box", "sphere", "cylinder", "capsule", "boxcap")


def tsp_cases(name):
    """Yaw-only cases of one TaskSpacePlanner scene: (pair, feature, target, yaw, d, anchor)."""
    up, side = (0.0, 0.0, 1.0), (1.0, 0.25, 0.0)
    lat = (0.011, 0.007, 0.0)
    yaws = (0.0, 0.3, np.pi / 2)
    targets = {"up": (("box-box", "box_up"), ("box-box", "box_yaw")),
               "cb2": (("box-box", "box_up"), ("cylinder-box", "cyl_up"), ("cylinder-box", "cyl_up2")),
               "generic": (("box-box", "box_up"), ("cylinder-box", "cyl_up"), ("box-box", "box_tilt"),
                           ("cylinder-box", "cyl_tilt"), ("sphere-box", "ball")),
               "capsule": (("box-box", "box_up"), ("capsule-box", "cap_up"), ("capsule-box", "cap_tilt"))}[name]
    cs = []
    for k, (pair, target) in enumerate(targets):
        for i, yaw in enumerate(yaws):
            for dd, anchor, feat in ((up, lat, "top"), (side, (0.0, 0.0, 0.01), "side")):
                c = _case(pair, feat, target, q_yaw(yaw) if yaw else IDENT, dd, anchor)
                c["yaw"] = yaw
                cs.append(c)
    return cs


# ------------------------------------------------------------------ bisection
def _line(ref, c):
    """The line the case's root moves on.  Hooks of a case (tests/envelope_scenes.py; none of this
    module's cases sets one): "origin", a world point that stands in for the target's position (a
    plane touched far from its origin, a target that hangs on a mover); "offset", a function of the
    quaternion giving the world vector from the root to the geom that is to touch (the line is the
    geom's, the root's lies that vector back)."""
    g = ref.geom(c["target"])
    pos = np.asarray(c["origin"] if "origin" in c else ref.ref["geom_pos"][g], float)
    if "offset" in c:
        pos = pos - c["offset"](c["quat"])
    if c["frame"] == "target":
        M = ref_mat(ref, c["target"])
        return pos + M @ c["anchor"], M @ c["d"]
    return pos + c["anchor"], c["d"]


def _pose(ref, c, a, d, t):
    p = a + t * d
    if "pose" in c:   # a case's own qpos row from the moved root and the quaternion (two movers)
        return c["pose"](p, c["quat"])
    if ref.mode == 1:
        return np.array([p[0], p[1], p[2], c["yaw"]])
    return np.concatenate([p, c["quat"]])


def bisect_touch(ref, c, deep=False):
    """The parameters (lo, hi) between which the reference's decision changes on the case's line,
    to the last bit the 60 steps resolve: contact (deep contact) at lo, none at hi = touch(d)."""
    a, d = _line(ref, c)
    hit = (lambda t: ref.contacts(_pose(ref, c, a, d, t))[1] > 0) if deep else \
        (lambda t: ref.contacts(_pose(ref, c, a, d, t))[0] > 0)
    lo, hi = 0.0, c.get("t_clear", T_CLEAR)
    if not hit(lo) or hit(hi):
        raise AssertionError("case %s / %s on %s does not go from overlap to clear" % (c["pair"], c["feature"], c["target"]))
    for _ in range(N_BISECT):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if hit(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


def poses_of(ref, cases, deep=False):
    """Every case's poses: dict(q [n, D], off [n], case [n] (index into cases), d [n, 3],
    touch [len(cases)]); with a case that writes its own qpos row ("pose"), also back [n, D], each
    pose moved 1 m on along d (where the moved coordinates are is the case's to say)."""
    q, off, idx, dirs, touch, back = [], [], [], [], [], []
    own_rows = any("pose" in c for c in cases)
    for k, c in enumerate(cases):
        a, d = _line(ref, c)
        c["d_world"] = d
        t_lo, t = bisect_touch(ref, c, deep)
        touch.append(t)
        for o in offsets_of(c):
            at = (t_lo if np.signbit(o) else t) if o == 0.0 else t + o
            q.append(_pose(ref, c, a, d, at))
            off.append(o)
            idx.append(k)
            dirs.append(d)
            if own_rows:
                back.append(_pose(ref, c, a, d, at + 1.0))
    out = dict(q=np.array(q), off=np.array(off), case=np.array(idx), d=np.array(dirs), touch=np.array(touch))
    if own_rows:
        out["back"] = np.array(back)
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------ the set, once per process
def write_scene(root, name, scene):
    """The scene as authored (the product's loader) and with every fromto geom restated (the
    independent reader): the two paths."""
    st, bodies = scene
    path, ref_path = os.path.join(root, name + ".xml"), os.path.join(root, name + "_ref.xml")
    for p, ex in ((path, False), (ref_path, True)):
        if not os.path.exists(p):
            with open(p, "w") as f:
                f.write(CS.mjcf(st, bodies, as_explicit=ex))
    return path, ref_path


_MEMO = {}


def sspp_set(root, kind, margin):
    """(ref of the small table, cases, poses) of one SamplingPathPlanner scene and margin."""
    key = ("sspp", kind, margin)
    if key not in _MEMO:
        _, ref_path = write_scene(root, "bp_%s_m%g_small" % (kind, margin), sspp_scene(kind, margin, "small"))
        ref = Ref(ref_path, 0, 7)
        cases = sspp_cases(kind)
        _MEMO[key] = (ref, cases, poses_of(ref, cases))
    return _MEMO[key]


def tsp_set(root, name, deep):
    """(ref, cases, poses) of one TaskSpacePlanner scene at the contact (margin 0) or the deep
    threshold."""
    key = ("tsp", name, deep)
    if key not in _MEMO:
        _, ref_path = write_scene(root, "bp_tsp_%s" % name, tsp_scene(name))
        ref = Ref(ref_path, 1, "mover")
        cases = tsp_cases(name)
        _MEMO[key] = (ref, cases, poses_of(ref, cases, deep))
    return _MEMO[key]


# a sphere's centre inside a box, away from every threshold (dist <= -r): (sphere radius, box
# half extents, centre in the box frame)
SPHERE_INSIDE = ((0.03, BOX_UP, (0.02, -0.01, 0.03)), (0.08, BOX_TILT, (0.0, 0.0, 0.0)), (0.03, BOX_UP, (0.099, 0.0, 0.0)))
