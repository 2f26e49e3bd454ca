"""Articulated test worlds as Python dicts, and their MJCF — TEST INFRASTRUCTURE ONLY.

A world is dict(geoms=[...], bodies=[...], excludes=[(body1, body2), ...]); a body is
dict(name, pos, quat, free=False, joints=[...], geoms=[...], children=[...]); a joint is
dict(type="hinge"|"slide", axis, pos, ref, name); a geom is dict(name, type, size, pos, quat,
contype, conaffinity, margin).  Every field but name / type / size has a default.  mjcf() writes the
file the product loads (angles in radians, orientations as quaternions); tests/chain_ref.py reads
the same dict on its own.
"""
import numpy as np

PLANE, SPHERE, CAPSULE, CYLINDER, BOX = "plane", "sphere", "capsule", "cylinder", "box"


def _f(v):
    return " ".join(repr(float(x)) for x in np.asarray(v, float).reshape(-1))


def _geom_xml(g, ind):
    a = ['type="%s"' % g["type"], 'size="%s"' % _f(g["size"])]
    if "name" in g:
        a.insert(0, 'name="%s"' % g["name"])
    for k in ("pos", "quat"):
        if k in g:
            a.append('%s="%s"' % (k, _f(g[k])))
    for k in ("contype", "conaffinity"):
        if k in g:
            a.append('%s="%d"' % (k, g[k]))
    if "margin" in g:
        a.append('margin="%s"' % repr(float(g["margin"])))
    return "%s<geom %s/>" % (ind, " ".join(a))


def _body_xml(b, ind):
    a = ['name="%s"' % b["name"], 'pos="%s"' % _f(b.get("pos", (0, 0, 0)))]
    if "quat" in b:
        a.append('quat="%s"' % _f(b["quat"]))
    out = ["%s<body %s>" % (ind, " ".join(a))]
    if b.get("free"):
        out.append(ind + "  <freejoint/>")
    for j in b.get("joints", ()):
        ja = ['type="%s"' % j["type"]]
        if "name" in j:
            ja.insert(0, 'name="%s"' % j["name"])
        for k in ("axis", "pos"):
            if k in j:
                ja.append('%s="%s"' % (k, _f(j[k])))
        if "ref" in j:
            ja.append('ref="%s"' % repr(float(j["ref"])))
        out.append("%s  <joint %s/>" % (ind, " ".join(ja)))
    out += [_geom_xml(g, ind + "  ") for g in b.get("geoms", ())]
    for c in b.get("children", ()):
        out += _body_xml(c, ind + "  ")
    out.append(ind + "</body>")
    return out


def mjcf(world):
    out = ['<mujoco model="chain">', '  <compiler angle="radian"/>', "  <worldbody>"]
    out += [_geom_xml(g, "    ") for g in world.get("geoms", ())]
    for b in world.get("bodies", ()):
        out += _body_xml(b, "    ")
    out.append("  </worldbody>")
    if world.get("excludes"):
        out.append("  <contact>")
        out += ['    <exclude body1="%s" body2="%s"/>' % e for e in world["excludes"]]
        out.append("  </contact>")
    out.append("</mujoco>")
    return "\n".join(out) + "\n"


def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def _chain(links):
    """nest a list of bodies: each the only child of the one before"""
    for a, b in zip(links[:-1], links[1:]):
        a.setdefault("children", []).append(b)
    return links[0]


# ------------------------------------------------------------------ closed-form worlds
def planar_2r(l1=0.4, l2=0.3):
    """two hinges about z; elbow at l1 along link 1's x, the tip a sphere at l2 along link 2's x"""
    l1b = dict(name="l1", pos=(0, 0, 0.5), joints=[dict(type="hinge", axis=(0, 0, 1), name="j1")],
               geoms=[dict(name="g1", type=SPHERE, size=(0.02, 0, 0), pos=(l1, 0, 0))])
    l2b = dict(name="l2", pos=(l1, 0, 0), joints=[dict(type="hinge", axis=(0, 0, 1), name="j2")],
               geoms=[dict(name="tip", type=SPHERE, size=(0.02, 0, 0), pos=(l2, 0, 0))])
    return dict(bodies=[_chain([l1b, l2b])])


def offcentre_hinge():
    """a hinge about y whose anchor is (0.1, 0, 0.2) off the body's origin"""
    return dict(bodies=[dict(name="b", pos=(0.3, 0, 0.4), joints=[dict(type="hinge", axis=(0, 1, 0), pos=(0.1, 0, 0.2))],
                             geoms=[dict(name="g", type=SPHERE, size=(0.02, 0, 0))])])


def slider(ref=0.0):
    return dict(bodies=[dict(name="b", pos=(0.1, 0.2, 0.3), joints=[dict(type="slide", axis=(0, 3, 4), ref=ref)],
                             geoms=[dict(name="g", type=SPHERE, size=(0.02, 0, 0))])])


def hinge_ref(ref=0.7):
    return dict(bodies=[dict(name="b", pos=(0.1, 0.2, 0.3), joints=[dict(type="hinge", axis=(1, 0, 0), ref=ref)],
                             geoms=[dict(name="g", type=SPHERE, size=(0.02, 0, 0), pos=(0, 0.25, 0))])])


def rotated_parent():
    """a jointless parent turned a quarter about z; the child's hinge about its own x"""
    c = np.sqrt(0.5)
    child = dict(name="c", pos=(0.2, 0, 0), joints=[dict(type="hinge", axis=(1, 0, 0))],
                 geoms=[dict(name="g", type=SPHERE, size=(0.02, 0, 0), pos=(0, 0.3, 0))])
    return dict(bodies=[dict(name="p", pos=(0, 0, 0.5), quat=(c, 0, 0, c), children=[child])])


def universal():
    """two hinges on one body: about z, then about the turned y"""
    return dict(bodies=[dict(name="b", pos=(0, 0, 0.5),
                             joints=[dict(type="hinge", axis=(0, 0, 1)), dict(type="hinge", axis=(0, 1, 0))],
                             geoms=[dict(name="g", type=SPHERE, size=(0.02, 0, 0), pos=(0.3, 0, 0))])])


def free_base_hinge():
    arm = dict(name="arm", pos=(0, 0, 0.1), joints=[dict(type="hinge", axis=(0, 1, 0))],
               geoms=[dict(name="g", type=SPHERE, size=(0.02, 0, 0), pos=(0.3, 0, 0))])
    return dict(bodies=[dict(name="base", pos=(0.5, 0.5, 0.2), free=True,
                             geoms=[dict(name="bg", type=BOX, size=(0.1, 0.1, 0.05))], children=[arm])])


# ------------------------------------------------------------------ random arms
def random_arm(nj, seed, link=CAPSULE, free_base=False, tool=True):
    """nj links, one joint each (every third a slide), random axes, anchors and body frames, link
    lengths <= 0.5 m; a capsule (or box / cylinder) along each link and a sphere tool at the tip"""
    rng = np.random.default_rng(seed)
    links = []
    for i in range(nj):
        L = rng.uniform(0.15, 0.5)
        j = dict(type="slide" if i % 3 == 2 else "hinge", axis=_unit(rng.normal(size=3)),
                 pos=rng.uniform(-0.05, 0.05, 3), name="j%d" % i)
        if i % 4 == 1:
            j["ref"] = rng.uniform(-0.5, 0.5)
        size = {CAPSULE: (0.03, 0.5 * L - 0.04, 0), CYLINDER: (0.03, 0.5 * L - 0.02, 0),
                BOX: (0.03, 0.025, 0.5 * L - 0.02)}[link if isinstance(link, str) else link[i % len(link)]]
        kind = link if isinstance(link, str) else link[i % len(link)]
        b = dict(name="link%d" % i, pos=(0, 0, 0.0) if i == 0 else (0, 0, links[-1]["_L"]),
                 quat=_unit(rng.normal(size=4)) if i else (1, 0, 0, 0), joints=[j],
                 geoms=[dict(name="lg%d" % i, type=kind, size=size, pos=(0, 0, 0.5 * L))], _L=L)
        links.append(b)
    if tool:
        links[-1]["geoms"].append(dict(name="tool", type=SPHERE, size=(0.04, 0, 0), pos=(0, 0, links[-1]["_L"] + 0.03)))
    root = _chain(links)
    if free_base:
        root["pos"] = (0, 0, 0.06)
        # (a sphere under capsule links: every pair of such an arm is one tests/capsule_ref.py decides)
        bg = dict(name="bg", type=SPHERE, size=(0.07, 0, 0)) if link == CAPSULE else dict(name="bg", type=BOX,
                                                                                         size=(0.08, 0.08, 0.04))
        root = dict(name="base", pos=(0, 0, 0.3), free=True, geoms=[bg], children=[root])
    else:
        root["pos"] = (0, 0, 0.3)
    return dict(bodies=[root])


def strip(world):
    """the world without the generator's private fields"""
    def body(b):
        o = {k: v for k, v in b.items() if not k.startswith("_") and k != "children"}
        o["children"] = [body(c) for c in b.get("children", ())]
        return o
    w = dict(world)
    w["bodies"] = [body(b) for b in world.get("bodies", ())]
    return w


def obstacles():
    """a floor, a box and a capsule post beside the arm's base"""
    c = np.sqrt(0.5)
    return [dict(name="floor", type=PLANE, size=(0, 0, 1)),
            dict(name="crate", type=BOX, size=(0.15, 0.2, 0.25), pos=(0.55, 0.1, 0.25)),
            dict(name="post", type=CAPSULE, size=(0.05, 0.4, 0), pos=(-0.45, 0.3, 0.45)),
            dict(name="rail", type=CAPSULE, size=(0.04, 0.5, 0), pos=(0.0, -0.5, 0.7), quat=(c, 0, c, 0))]


def capsule_arm_world(nj=7, seed=11, free_base=False):
    """scene 1: a capsule-link arm with a sphere tool over a floor, beside a box and capsule posts"""
    w = strip(random_arm(nj, seed, CAPSULE, free_base))
    w["geoms"] = obstacles()
    return w


def box_cyl_arm_world(nj=5, seed=5):
    """scene 2: box and cylinder links (every pair type capsule_ref lacks) beside a box, a cylinder
    and a sphere over a floor: decided through the frozen twin"""
    w = strip(random_arm(nj, seed, (BOX, CYLINDER), False, tool=True))
    w["geoms"] = [dict(name="floor", type=PLANE, size=(0, 0, 1)),
                  dict(name="crate", type=BOX, size=(0.15, 0.2, 0.25), pos=(0.5, 0.1, 0.25)),
                  dict(name="drum", type=CYLINDER, size=(0.12, 0.3, 0), pos=(-0.4, 0.3, 0.3)),
                  dict(name="ball", type=SPHERE, size=(0.15, 0, 0), pos=(0.0, -0.5, 0.6))]
    return w


def arm_poses(D, n, seed, spread=2.0, free_base=False):
    """n poses of D values for random_arm's joints: uniform in +-spread (a slide, every third
    joint: scaled by 0.15); a free base's 7 values: x, y in +-0.2, z in 0.05 .. 0.5, a random quaternion"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-spread, spread, (n, D))
    j0 = 7 if free_base else 0
    for d in range(j0, D):
        if (d - j0) % 3 == 2:
            q[:, d] *= 0.15
    if free_base:
        base = np.concatenate([rng.uniform(-0.2, 0.2, (n, 2)), rng.uniform(0.05, 0.5, (n, 1)), rng.normal(size=(n, 4))], 1)
        q[:, :min(7, D)] = base[:, :min(7, D)]
    return np.ascontiguousarray(q)
