"""Synthetic MJCF scenes for tests/test_gpu_synthetic_scenes.py — TEST INFRASTRUCTURE ONLY.

The three shipped scenes have no sphere, only the identity plane, one (mover) cylinder and at
most 48 pairs.  The scenes authored here put the other primitives, tilted planes, static
cylinders, more than 64 pairs, far-away statics and a second mover in front of the device
kernels.  Each scene is a list of static geoms (world body) plus free bodies, written as an
MJCF string that uses only what both loaders read the same way: <compiler angle="radian"/>,
pos, quat, size, contype, conaffinity, margin, <freejoint/>.
"""
import numpy as np

PLANE, SPHERE, CYLINDER, BOX = 0, 2, 5, 6
_TYPE_NAMES = {PLANE: "plane", SPHERE: "sphere", CYLINDER: "cylinder", BOX: "box"}

# the plane every scene but TSP (ii)/(iii) stands on: tilted about x by 0.2 rad, below the origin
RAMP_QUAT = (0.9950, 0.0998, 0.0, 0.0)
RAMP_POS = (0.0, 0.0, -0.05)


def geom(type, size, pos=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0), name="", contype=1,
         conaffinity=1, margin=0.0):
    size = (size,) if np.isscalar(size) else tuple(size)
    return dict(type=type, size=tuple(float(x) for x in size), pos=tuple(float(x) for x in pos),
                quat=tuple(float(x) for x in quat), name=name, contype=int(contype),
                conaffinity=int(conaffinity), margin=float(margin))


def ramp(**kw):
    return geom(PLANE, (0, 0, 1), RAMP_POS, RAMP_QUAT, name="ramp", **kw)


def body(name, pos, geoms, quat=(1.0, 0.0, 0.0, 0.0)):
    return dict(name=name, pos=tuple(float(x) for x in pos), quat=tuple(float(x) for x in quat),
                geoms=list(geoms))


def _vec(v):
    return " ".join(repr(float(x)) for x in v)


def _geom_xml(g):
    s = '<geom type="%s" size="%s" pos="%s" quat="%s"' % (_TYPE_NAMES[g["type"]], _vec(g["size"]),
                                                          _vec(g["pos"]), _vec(g["quat"]))
    if g["name"]:
        s += ' name="%s"' % g["name"]
    if g["contype"] != 1:
        s += ' contype="%d"' % g["contype"]
    if g["conaffinity"] != 1:
        s += ' conaffinity="%d"' % g["conaffinity"]
    if g["margin"]:
        s += ' margin="%s"' % repr(g["margin"])
    return s + "/>"


def mjcf(statics, bodies):
    """Statics first (world body), then one free body per entry: the free bodies' qpos lead."""
    out = ['<mujoco>', '  <compiler angle="radian"/>', '  <worldbody>']
    out += ["    " + _geom_xml(g) for g in statics]
    for b in bodies:
        out.append('    <body name="%s" pos="%s" quat="%s">' % (b["name"], _vec(b["pos"]), _vec(b["quat"])))
        out.append('      <freejoint/>')
        out += ["      " + _geom_xml(g) for g in b["geoms"]]
        out.append('    </body>')
    out += ['  </worldbody>', '</mujoco>']
    return "\n".join(out) + "\n"


def shifted(statics, d):
    """The statics translated rigidly by d."""
    return [dict(g, pos=tuple(p + x for p, x in zip(g["pos"], d))) for g in statics]


def with_geoms_off(ref, off):
    """A copy of a mjcf_ref model with the geoms `off` (indices) made non-collidable."""
    m = dict(ref)
    mask = np.zeros(len(ref["geom_type"]), bool)
    mask[list(off)] = True
    m["geom_contype"] = np.where(mask, 0, ref["geom_contype"])
    m["geom_conaffinity"] = np.where(mask, 0, ref["geom_conaffinity"])
    return m


def geoms_named(ref, prefix):
    return [i for i, n in enumerate(ref["geom_names"]) if n.startswith(prefix)]


def assert_loaders_agree(arrays, ref):
    """The product loader's arrays against the independent reader's, every array (geom types,
    sizes, bits, margins, geom and body poses, qpos0), as
    test_scenes_capi.test_loader_matches_independent_reader does.  The scenes' bodies all hang
    off the world, so equal body and geom poses are equal world poses."""
    for k, v in arrays.items():
        v = np.asarray(v)
        np.testing.assert_array_equal(v, np.asarray(ref[k]).reshape(v.shape), err_msg=k)


# ------------------------------------------------------------------ the FP32 filter's range
def _rbound(t, s):
    if t == BOX:
        return float(np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]))
    if t == CYLINDER:
        return float(np.sqrt(s[0] * s[0] + s[1] * s[1]))
    if t == SPHERE:
        return float(s[0])
    return 0.0


def moving_pairs(ref, dof):
    """(moving geom, other geom) index pairs of the qpos window [0, dof): the bit filter and the
    same-body rule restated for scenes whose bodies all hang off the world."""
    mv = [b for b in range(len(ref["body_parent"])) if 0 <= ref["body_qpos_adr"][b] < dof]
    gb, ct, ca = ref["geom_body"], ref["geom_contype"], ref["geom_conaffinity"]
    out = []
    for g1 in range(len(gb)):
        for g2 in range(g1 + 1, len(gb)):
            if gb[g1] == gb[g2] or not (gb[g1] in mv or gb[g2] in mv):
                continue
            if not ((ct[g1] & ca[g2]) or (ct[g2] & ca[g1])):
                continue
            out.append((g1, g2) if gb[g1] in mv else (g2, g1))
    return out


def expected_scan(ref, dof):
    """What the library's f32_eps rule says about a scene's pair table: the FP32-filtered scan
    for at most 64 pairs, every pair extent (bounding radii + margin + the moving geom's offset
    from its root) at most 8 m and every static within 16 m of the origin per axis; else FP64."""
    pairs = moving_pairs(ref, dof)
    if not pairs or len(pairs) > 64:
        return "fp64"
    mv = [b for b in range(len(ref["body_parent"])) if 0 <= ref["body_qpos_adr"][b] < dof]
    for gm, go in pairs:
        ext = (_rbound(ref["geom_type"][gm], ref["geom_size"][gm]) + _rbound(ref["geom_type"][go], ref["geom_size"][go]) +
               max(ref["geom_margin"][gm], ref["geom_margin"][go]) + float(np.linalg.norm(ref["geom_pos"][gm])))
        far = float(np.abs(ref["geom_pos"][go]).max())  # (a mover partner's offset from its root)
        if not ext <= 8.0 or (ref["geom_body"][go] not in mv and not far <= 16.0):
            return "fp64"
    return "fp32-filtered"


# ------------------------------------------------------------------ scenes
MOVER_BOX = (0.04, 0.03, 0.02)


def zoo():
    """Case 1: every primitive on both sides.  The mover cylinder (contype = conaffinity = 2) and
    the static cylinder (1 / 1) share no bit: that pair, which no narrowphase supports, is
    filtered; the other statics carry both bits (3 / 3)."""
    statics = [ramp(contype=3, conaffinity=3),
               geom(SPHERE, 0.08, (0.25, 0.1, 0.15), name="ball", contype=3, conaffinity=3),
               geom(CYLINDER, (0.05, 0.12), (0.5, -0.1, 0.2), (0.92, 0.3, 0.2, 0.1), name="post"),
               geom(BOX, (0.06, 0.1, 0.04), (0.75, 0.05, 0.18), (0.8, 0.1, 0.5, 0.3), name="slab",
                    contype=3, conaffinity=3)]
    mover = body("mover", (0, 0, 0.3), [
        geom(BOX, MOVER_BOX, name="m_box"),
        geom(SPHERE, 0.03, (0.07, 0, 0.01), name="m_ball"),
        geom(CYLINDER, (0.025, 0.04), (-0.07, 0.01, 0), (0.7, 0.7, 0.1, 0), name="m_cyl", contype=2,
             conaffinity=2, margin=0.002)])
    return mjcf(statics, [mover])


ZOO_START = np.array([0.0, 0.0, 0.22, 1, 0, 0, 0])
ZOO_END = np.array([1.0, 0.0, 0.22, 1, 0, 0, 0])
ZOO_LIMITS = np.array([1, 1, 1, .3, .3, .3, .3])


def one_type_statics(kind):
    if kind == "spheres":
        return [geom(SPHERE, 0.07, (0.1, 0.14, 0.16), name="s0"),
                geom(SPHERE, 0.05, (0.25, -0.13, 0.24), name="s1"),
                geom(SPHERE, 0.09, (0.4, 0.02, 0.32), name="s2")]
    if kind == "boxes":
        return [geom(BOX, (0.06, 0.1, 0.04), (0.1, 0.17, 0.16), (0.8, 0.1, 0.5, 0.3), name="b0"),
                geom(BOX, (0.05, 0.05, 0.08), (0.25, -0.15, 0.26), (0.9, -0.3, 0.2, 0.2), name="b1"),
                geom(BOX, (0.09, 0.04, 0.05), (0.4, 0.03, 0.32), (0.6, 0.5, -0.4, 0.1), name="b2")]
    if kind == "cylinders":
        return [geom(CYLINDER, (0.05, 0.12), (0.15, 0.08, 0.2), name="c_up"),
                geom(CYLINDER, (0.04, 0.15), (0.35, -0.1, 0.25), (0.92, 0.3, 0.2, 0.1), name="c_tilt")]
    raise ValueError(kind)


def one_type(kind, shift=(0.0, 0.0, 0.0), mirror=False):
    """Case 2 (and 4, shifted): a single-geom box mover over the tilted plane and statics of one
    kind.  mirror: a second copy of the statics reflected to the other side, along -y."""
    st = [ramp()] + one_type_statics(kind)
    st = shifted(st, shift)
    if mirror:
        st += [dict(g, name=g["name"] + "_m", pos=(g["pos"][0], -g["pos"][1] - 15.6, g["pos"][2]))
               for g in st[1:]]
    return mjcf(st, [body("mover", (shift[0], shift[1], 0.3 + shift[2]), [geom(BOX, MOVER_BOX, name="m_box")])])


def hull_cull():
    """Case 1b: 12 pairs (three moving geoms x the tilted plane and three spheres), the fewest
    statics that keep the survivors' hull masks on (9 to 64 pairs), for a job whose candidates
    spread widely along y: the plane's normal has a y component, so the plane branch of
    pair_may_touch must pick the right end of the control points' y range."""
    mover = body("mover", (0, 0, 0.3), [geom(BOX, MOVER_BOX, name="m_box"),
                                        geom(SPHERE, 0.03, (0.07, 0, 0.01), name="m_ball"),
                                        geom(SPHERE, 0.025, (-0.06, 0.02, 0), name="m_ball2")])
    return mjcf([ramp()] + one_type_statics("spheres"), [mover])


HULL_LIMITS = np.array([1, 3, 1, .3, .3, .3, .3])
ONE_START = np.array([0.0, 0.0, 0.16, 1, 0, 0, 0])
ONE_END = np.array([0.5, 0.0, 0.16, 1, 0, 0, 0])


def big_table():
    """Case 4, the extent edge: the boxes scene over a table whose bounding radius passes 8 m."""
    st = [ramp()] + one_type_statics("boxes") + [geom(BOX, (6.0, 6.0, 0.05), (0.25, 0.0, 0.02), name="table")]
    return mjcf(st, [body("mover", (0, 0, 0.3), [geom(BOX, MOVER_BOX, name="m_box")])])


def grid(n_mover, n_static):
    """Case 3: n_static static boxes at general rotations — all but the last on a jittered grid
    beside the path, the last one alone under the path's centre line — and a mover of n_mover
    small boxes with their own rotations (relrot), the last of them hanging below the others:
    the last pair of the table (last mover geom, last static) is some candidates' only contact."""
    rng = np.random.default_rng(1000 * n_mover + n_static)
    st = []
    cols = n_static // 2
    for i in range(n_static):
        r, c = divmod(i, cols)
        pos = (0.1 + 0.9 * c / max(cols - 1, 1) + rng.uniform(-0.02, 0.02),
               (-0.09 if r == 0 else 0.09) + rng.uniform(-0.02, 0.02), 0.12 + rng.uniform(-0.04, 0.04))
        if i == n_static - 1:
            pos = (0.55, 0.0, 0.1)
        q = rng.normal(size=4)
        st.append(geom(BOX, (0.02, 0.025, 0.03), pos, q / np.linalg.norm(q), name="st%02d" % i))
    mg = []
    for k in range(n_mover):
        q = rng.normal(size=4)
        a = 2 * np.pi * k / n_mover
        pos = (0.04 * np.cos(a), 0.04 * np.sin(a), 0.01 * (k % 2))
        if k == n_mover - 1:
            pos = (0.0, 0.0, -0.04)
        mg.append(geom(BOX, (0.015, 0.01, 0.012), pos, q / np.linalg.norm(q), name="mv%d" % k))
    return mjcf(st, [body("mover", (0, 0, 0.3), mg)])


GRID_START = np.array([0.0, 0.0, 0.2, 1, 0, 0, 0])
GRID_END = np.array([1.1, 0.0, 0.2, 1, 0, 0, 0])


def two_movers():
    """Case 5: two free bodies lead qpos; a D = 9 window moves body 0 fully and body 1 in x, y
    (its z and rotation stay at qpos0)."""
    st = [geom(SPHERE, 0.07, (0.3, 0.12, 0.25), name="ball"),
          geom(BOX, (0.05, 0.08, 0.04), (0.7, -0.1, 0.22), (0.8, 0.1, 0.5, 0.3), name="slab")]
    b0 = body("m0", (0, 0, 0.3), [geom(BOX, MOVER_BOX, name="a_box"),
                                    geom(SPHERE, 0.03, (0.07, 0, 0.01), name="a_ball")])
    b1 = body("m1", (0.5, 0.1, 0.24), [geom(BOX, (0.05, 0.04, 0.03), name="b_box"),
                                         geom(SPHERE, 0.035, (0, 0.07, 0.0), name="b_ball")],
              quat=(0.9, 0.1, -0.2, 0.3))
    return mjcf(st, [b0, b1])


TWO_START = np.array([0.0, 0.0, 0.25, 1, 0, 0, 0, 0.5, 0.1])
TWO_END = np.array([1.0, 0.0, 0.25, 1, 0, 0, 0, 0.5, -0.1])


def tsp_boxes():
    """Case 6 (i): yaw-only box mover; one upright and one non-upright static box (the job's
    box-box narrowphase cannot be the upright one), a sphere and the tilted plane."""
    st = [ramp(),
          geom(BOX, (0.05, 0.05, 0.1), (0.0, 0.15, 0.1), (0.9239, 0, 0, 0.3827), name="up"),
          geom(BOX, (0.05, 0.07, 0.06), (0.0, -0.15, 0.15), (0.8, 0.1, 0.5, 0.3), name="tilt"),
          geom(SPHERE, 0.07, (0.15, 0.0, 0.25), name="ball")]
    return mjcf(st, [body("mover", (-0.3, 0, 0.2), [geom(BOX, (0.03, 0.03, 0.03), name="m_box")])])


def tsp_cylinders(tilted):
    """Case 6 (ii) / (iii): box mover, static cylinders only — all vertical (ii), or one of them
    tilted (iii) — over a flat plane."""
    q = (0.92, 0.3, 0.2, 0.1) if tilted else (1.0, 0.0, 0.0, 0.0)
    st = [geom(PLANE, (0, 0, 1), name="floor"),
          geom(CYLINDER, (0.05, 0.12), (0.0, 0.12, 0.12), name="c0"),
          geom(CYLINDER, (0.04, 0.15), (0.05, -0.12, 0.15), q, name="c1"),
          geom(CYLINDER, (0.06, 0.08), (0.2, 0.02, 0.3), name="c2")]
    return mjcf(st, [body("mover", (-0.3, 0, 0.2), [geom(BOX, (0.03, 0.03, 0.03), name="m_box")])])


TSP_START = np.array([-0.3, 0.0, 0.2, 0.0])
TSP_END = np.array([0.35, 0.0, 0.2, 0.8])
TSP_LO, TSP_HI = np.array([-0.5, -0.5, 0.0, -1.6]), np.array([0.5, 0.5, 0.6, 1.6])
