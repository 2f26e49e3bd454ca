"""numpy reference for articulated movers — TEST INFRASTRUCTURE ONLY.

Written from the rule of DESIGN.md §5 "Articulated movers" (MuJoCo's mj_kinematics), on the world
dicts of tests/chain_scenes.py, sharing no code with the product: the model arrays (flatten), forward
kinematics vectorised over N poses (fk), the pair filter (pairs) and the contact decisions (contacts)
from tests/capsule_ref.py's colliders plus plane-sphere, sphere-sphere and sphere-box written out
here.  For the other pair types the reference is the frozen twin (twin_world): every link a
top-level free body at this module's FK pose, decided by the scene builder's env-env path.
"""
import numpy as np

from tests import capsule_ref as CR

TYPE = {"plane": 0, "sphere": 2, "capsule": 3, "cylinder": 5, "box": 6}
NAME = {v: k for k, v in TYPE.items()}
NEAR = 1e-9


def _unitq(q):
    q = np.asarray(q, float)
    return q / np.linalg.norm(q)


def flatten(world):
    """MuJoCo-like arrays: bodies in depth-first pre-order (world = 0), geoms body by body, joints in
    body order; qpos: 7 per free joint, 1 per hinge / slide."""
    m = dict(body_parent=[-1], body_pos=[np.zeros(3)], body_quat=[np.array([1.0, 0, 0, 0])], body_names=["world"],
             body_free=[-1], body_joints=[[]], jnt_type=[], jnt_body=[], jnt_adr=[], jnt_axis=[], jnt_pos=[],
             qpos0=[], geoms=[], exclude=[])
    per_body = {0: list(world.get("geoms", ()))}

    def walk(b, parent):
        bid = len(m["body_parent"])
        m["body_parent"].append(parent)
        m["body_pos"].append(np.asarray(b.get("pos", (0, 0, 0)), float))
        m["body_quat"].append(_unitq(b.get("quat", (1, 0, 0, 0))))
        m["body_names"].append(b["name"])
        m["body_free"].append(-1)
        m["body_joints"].append([])
        if b.get("free"):
            m["body_free"][bid] = len(m["qpos0"])
            m["qpos0"] += list(m["body_pos"][bid]) + list(m["body_quat"][bid])
        for j in b.get("joints", ()):
            m["body_joints"][bid].append(len(m["jnt_type"]))
            m["jnt_type"].append(2 if j["type"] == "slide" else 3)
            m["jnt_body"].append(bid)
            m["jnt_adr"].append(len(m["qpos0"]))
            a = np.asarray(j.get("axis", (0, 0, 1)), float)
            m["jnt_axis"].append(a / np.linalg.norm(a))
            m["jnt_pos"].append(np.asarray(j.get("pos", (0, 0, 0)), float))
            m["qpos0"].append(float(j.get("ref", 0.0)))
        per_body[bid] = list(b.get("geoms", ()))
        for c in b.get("children", ()):
            walk(c, bid)

    for b in world.get("bodies", ()):
        walk(b, 0)
    for bid in range(len(m["body_parent"])):
        for g in per_body[bid]:
            s = list(g["size"]) + [0.0] * (3 - len(g["size"]))
            m["geoms"].append(dict(name=g.get("name", ""), type=TYPE[g["type"]], body=bid, size=np.asarray(s, float),
                                   pos=np.asarray(g.get("pos", (0, 0, 0)), float),
                                   quat=_unitq(g.get("quat", (1, 0, 0, 0))), contype=g.get("contype", 1),
                                   conaffinity=g.get("conaffinity", 1), margin=float(g.get("margin", 0.0))))
    for b1, b2 in world.get("excludes", ()):
        m["exclude"].append((m["body_names"].index(b1), m["body_names"].index(b2)))
    m["qpos0"] = np.asarray(m["qpos0"], float)
    m["nq"] = len(m["qpos0"])
    return m


# ------------------------------------------------------------------ quaternions, vectorised [N, 4]
def qmul(a, b):
    a0, a1, a2, a3 = np.moveaxis(a, -1, 0)
    b0, b1, b2, b3 = np.moveaxis(b, -1, 0)
    return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                     a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], -1)


def qmat(q):
    """rotation matrices [N, 3, 3] of (not necessarily unit) quaternions, MuJoCo's mju_quat2Mat"""
    w, x, y, z = np.moveaxis(q, -1, 0)
    return np.stack([np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)], -2)


def rot(q, v):
    return np.einsum("nij,nj->ni", qmat(q), np.broadcast_to(v, q.shape[:-1] + (3,)))


def full_qpos(m, q):
    """SamplingPathPlanner's pose rule: q[0:D] -> qpos[0:D], the rest at qpos0"""
    q = np.asarray(q, float)
    out = np.tile(m["qpos0"], (len(q), 1))
    out[:, :q.shape[1]] = q
    return out


def fk(m, qpos):
    """mj_kinematics over N poses: (xpos [N, nb, 3], xquat [N, nb, 4], gpos [N, ng, 3], gmat [N, ng, 9])"""
    qpos = np.asarray(qpos, float)
    N, nb = len(qpos), len(m["body_parent"])
    xpos, xquat = np.zeros((N, nb, 3)), np.zeros((N, nb, 4))
    xquat[:, 0, 0] = 1.0
    for b in range(1, nb):
        fa = m["body_free"][b]
        if fa >= 0:
            p, q = qpos[:, fa:fa + 3].copy(), qpos[:, fa + 3:fa + 7].copy()
        else:
            pa = m["body_parent"][b]
            p = xpos[:, pa] + rot(xquat[:, pa], m["body_pos"][b])
            q = qmul(xquat[:, pa], np.broadcast_to(m["body_quat"][b], (N, 4)))
            for j in m["body_joints"][b]:
                adr = m["jnt_adr"][j]
                a = qpos[:, adr] - m["qpos0"][adr]
                anchor = p + rot(q, m["jnt_pos"][j])
                if m["jnt_type"][j] == 2:
                    p = p + rot(q, m["jnt_axis"][j]) * a[:, None]
                else:
                    ql = np.concatenate([np.cos(0.5 * a)[:, None], np.sin(0.5 * a)[:, None] * m["jnt_axis"][j]], 1)
                    q = qmul(q, ql)
                    p = anchor - rot(q, m["jnt_pos"][j])
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        xpos[:, b], xquat[:, b] = p, q
    ng = len(m["geoms"])
    gpos, gmat = np.zeros((N, ng, 3)), np.zeros((N, ng, 9))
    for g, G in enumerate(m["geoms"]):
        b = G["body"]
        gpos[:, g] = xpos[:, b] + rot(xquat[:, b], G["pos"])
        gq = qmul(xquat[:, b], np.broadcast_to(G["quat"], (N, 4)))
        gq = gq / np.linalg.norm(gq, axis=1, keepdims=True)
        gmat[:, g] = qmat(gq).reshape(N, 9)
    return xpos, xquat, gpos, gmat


# ------------------------------------------------------------------ pair filter
def driven_bodies(m, D):
    nb = len(m["body_parent"])
    d = [False] * nb
    for b in range(1, nb):
        d[b] = d[m["body_parent"][b]] or (0 <= m["body_free"][b] < D) or any(m["jnt_adr"][j] < D for j in m["body_joints"][b])
    return d


def welds(m):
    nb = len(m["body_parent"])
    w = [0] * nb
    for b in range(1, nb):
        w[b] = b if (m["body_free"][b] >= 0 or m["body_joints"][b]) else w[m["body_parent"][b]]
    return w


def all_pairs(m):
    """the filter's pairs (g1 < g2): same weld skipped, parent-child welds skipped unless one is the
    world, <exclude>, contype / conaffinity; margin = the larger one"""
    w, G = welds(m), m["geoms"]
    out = []
    for g1 in range(len(G)):
        for g2 in range(g1 + 1, len(G)):
            b1, b2 = G[g1]["body"], G[g2]["body"]
            w1, w2 = w[b1], w[b2]
            if w1 == w2:
                continue
            if not ((G[g1]["contype"] & G[g2]["conaffinity"]) or (G[g2]["contype"] & G[g1]["conaffinity"])):
                continue
            if w1 and w2 and (w1 == w[m["body_parent"][w2]] or w2 == w[m["body_parent"][w1]]):
                continue
            if (b1, b2) in m["exclude"] or (b2, b1) in m["exclude"]:
                continue
            out.append((g1, g2, max(G[g1]["margin"], G[g2]["margin"])))
    return out


def pairs(m, D):
    """(moving pairs, static-static pairs) for the pose rule of D values"""
    d = driven_bodies(m, D)
    mv = [p for p in all_pairs(m) if d[m["geoms"][p[0]]["body"]] or d[m["geoms"][p[1]]["body"]]]
    st = [p for p in all_pairs(m) if not (d[m["geoms"][p[0]]["body"]] or d[m["geoms"][p[1]]["body"]])]
    return mv, st


# ------------------------------------------------------------------ contact decisions
def rbound(G):
    t, s = G["type"], G["size"]
    return {0: 0.0, 2: s[0], 3: s[0] + s[1], 5: np.hypot(s[0], s[1]), 6: np.linalg.norm(s)}[t]


def pair_dist(t1, p1, m1, s1, t2, p2, m2, s2, margin):
    """signed distances [N, k] of the sphere tests the pair's rule runs (nan: not run), geom 1 first
    by (type, index); contact iff some dist <= margin"""
    N = len(p1)
    S1, S2 = np.tile(s1, (N, 1)), np.tile(s2, (N, 1))
    if t1 == 0 and t2 == 2:
        return (CR.dot(CR.zcol(m1), p2 - p1) - s2[0])[:, None]
    if t1 == 2 and t2 == 2:
        return (np.linalg.norm(p2 - p1, axis=1) - (s1[0] + s2[0]))[:, None]
    if t1 == 2 and t2 == 6:
        loc = CR.to_frame(m2, p1 - p2)
        out = np.abs(loc) - s2
        outside = np.linalg.norm(np.maximum(out, 0.0), axis=1)
        inside = out.max(1)
        return (np.where((out <= 0).all(1), inside, outside) - s1[0])[:, None]
    return CR.collide(t1, p1, m1, S1, t2, p2, m2, S2, margin)[2]


def contacts(m, D, q):
    """(hit [N] bool, near [N] bool, per-pair contact [N, P] bool): near marks a pose where some
    pair's decisive distance lies within NEAR of its margin"""
    _, _, gpos, gmat = fk(m, full_qpos(m, q))
    mv, _ = pairs(m, D)
    N = len(gpos)
    hit, near = np.zeros((N, len(mv)), bool), np.zeros(N, bool)
    for k, (g1, g2, margin) in enumerate(mv):
        A, B = m["geoms"][g1], m["geoms"][g2]
        a, b = (g1, g2) if A["type"] <= B["type"] else (g2, g1)
        A, B = m["geoms"][a], m["geoms"][b]
        d = pair_dist(A["type"], gpos[:, a], gmat[:, a], A["size"], B["type"], gpos[:, b], gmat[:, b], B["size"], margin)
        c = (d <= margin).any(1)
        ra, rb = rbound(A), rbound(B)
        if ra > 0 and rb > 0:
            cull = ((gpos[:, b] - gpos[:, a]) ** 2).sum(1) > (ra + rb + margin) ** 2
            assert not (c & cull).any()  # (the broadphase is conservative)
            c &= ~cull
        hit[:, k] = c
        near |= np.nanmin(np.abs(d - margin), 1) < NEAR
    return hit.any(1), near, hit


# ------------------------------------------------------------------ the frozen twin
def twin_world(world, m):
    """The same geoms with every body a top-level free body (its pose comes per pose from fk), the
    parent-child rule and the same-weld rule restated as <exclude>s."""
    w = welds(m)
    nb = len(m["body_parent"])
    per_body = {b: [] for b in range(nb)}
    for G in m["geoms"]:
        per_body[G["body"]].append(dict(name=G["name"], type=NAME[G["type"]], size=tuple(G["size"]), pos=tuple(G["pos"]),
                                        quat=tuple(G["quat"]), contype=G["contype"], conaffinity=G["conaffinity"],
                                        margin=G["margin"]))
    bodies = [dict(name=m["body_names"][b], free=True, geoms=per_body[b]) for b in range(1, nb)]
    ex = [(m["body_names"][x], m["body_names"][y]) for x, y in m["exclude"]]
    for b1 in range(1, nb):
        for b2 in range(b1 + 1, nb):
            w1, w2 = w[b1], w[b2]
            if w1 == w2 or (w1 and w2 and (w1 == w[m["body_parent"][w2]] or w2 == w[m["body_parent"][w1]])):
                ex.append((m["body_names"][b1], m["body_names"][b2]))
    return dict(geoms=per_body[0], bodies=bodies, excludes=ex)


def twin_qpos(m, q):
    """the twin's qpos [N, 7 (nb - 1)] at the chain poses q"""
    xpos, xquat, _, _ = fk(m, full_qpos(m, q))
    return np.ascontiguousarray(np.concatenate([xpos[:, 1:], xquat[:, 1:]], 2).reshape(len(xpos), -1))
