"""numpy reference for worlds of arms — TEST INFRASTRUCTURE ONLY.

Written from the rule of DESIGN.md §5 "Worlds for arms", no product code: the pose rule is
q[0:D] -> qpos[0:D], the rest from the world, so the kinematics are tests/chain_ref.py's fk on
full = world overwritten by q[0:D] (qpos0 stays every joint's zero inside fk), on model arrays whose
body_pos / body_quat hold the world's body poses.  Decisions: chain_ref.pairs and pair_dist, plus the
plane-box test written out here; a static box-box pair is decided only where the bounding spheres
already separate it.
"""
import copy

import numpy as np

from tests import capsule_ref as CR
from tests import chain_ref as R

NEAR = R.NEAR


def model(world_dict, poses=()):
    """chain_ref's arrays with the bodies of poses = [(name, pos, quat)] re-posed in order (a free
    body's pose is returned as its 7 qpos values instead: see world_qpos)"""
    m = copy.deepcopy(R.flatten(world_dict))
    for name, pos, quat in poses:
        b = m["body_names"].index(name)
        if m["body_free"][b] < 0:
            m["body_pos"][b] = np.asarray(pos, float)
            m["body_quat"][b] = np.asarray(quat, float) / np.linalg.norm(quat)
    return m


def world_qpos(m, qpos=None, poses=()):
    """the world's qpos: the model's own or qpos, free-joint quaternions normalised, then the free
    bodies among poses"""
    w = m["qpos0"].copy() if qpos is None else np.asarray(qpos, float).copy()
    for b, fa in enumerate(m["body_free"]):
        if fa >= 0:
            w[fa + 3:fa + 7] /= np.linalg.norm(w[fa + 3:fa + 7])
    for name, pos, quat in poses:
        fa = m["body_free"][m["body_names"].index(name)]
        if fa >= 0:
            w[fa:fa + 3] = pos
            w[fa + 3:fa + 7] = np.asarray(quat, float) / np.linalg.norm(quat)
    return w


def full_qpos(world, q, D):
    q = np.asarray(q, float).reshape(-1, D)
    out = np.tile(np.asarray(world, float), (len(q), 1))
    out[:, :D] = q
    return out


def fk(m, world, q, D):
    """(gpos [N, ng, 3], gmat [N, ng, 9]) of the poses q [N, D] in the world"""
    _, _, gpos, gmat = R.fk(m, full_qpos(world, q, D))
    return gpos, gmat


def _plane_box(pp, pm, bp, bm, be):
    """signed distances [N, 8] of the box's corners to the plane"""
    n = CR.zcol(pm)
    B = bm.reshape(-1, 3, 3)
    out = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                c = bp + np.einsum("nij,j->ni", B, np.array([sx, sy, sz]) * be)
                out.append(CR.dot(n, c - pp))
    return np.stack(out, 1)


def _decide(m, gpos, gmat, g1, g2, margin):
    """(contact [N] bool, near [N] bool) of one pair, geom a first by (type, index)"""
    A, B = m["geoms"][g1], m["geoms"][g2]
    a, b = (g1, g2) if A["type"] <= B["type"] else (g2, g1)
    A, B = m["geoms"][a], m["geoms"][b]
    ra, rb = R.rbound(A), R.rbound(B)
    far = np.zeros(len(gpos), bool)
    if ra > 0 and rb > 0:
        far = ((gpos[:, b] - gpos[:, a]) ** 2).sum(1) > (ra + rb + margin) ** 2
    if (A["type"], B["type"]) == (0, 6):
        d = _plane_box(gpos[:, a], gmat[:, a], gpos[:, b], gmat[:, b], B["size"])
    elif (A["type"], B["type"]) == (6, 6):
        assert far.all(), "a box-box pair the bounding spheres do not separate: not decided here"
        return np.zeros(len(gpos), bool), np.zeros(len(gpos), bool)
    else:
        d = R.pair_dist(A["type"], gpos[:, a], gmat[:, a], A["size"], B["type"], gpos[:, b], gmat[:, b], B["size"], margin)
    c = (d <= margin).any(1)
    assert not (c & far).any()  # (the broadphase is conservative)
    return c & ~far, np.nanmin(np.abs(d - margin), 1) < NEAR


def contacts(m, D, world, q):
    """(hit [N] bool, near [N] bool, per-pair contact [N, P] bool) over the moving pairs"""
    gpos, gmat = fk(m, world, q, D)
    mv, _ = R.pairs(m, D)
    hit, near = np.zeros((len(gpos), len(mv)), bool), np.zeros(len(gpos), bool)
    for k, (g1, g2, margin) in enumerate(mv):
        hit[:, k], nr = _decide(m, gpos, gmat, g1, g2, margin)
        near |= nr
    return hit.any(1), near, hit


def static_contacts(m, D, world):
    """([(g1, g2, contact bool)], near bool) over the static-static pairs at the world's poses"""
    gpos, gmat = fk(m, world, np.asarray(world, float)[None, :D], D)
    out, near = [], False
    for g1, g2, margin in R.pairs(m, D)[1]:
        c, nr = _decide(m, gpos, gmat, g1, g2, margin)
        out.append((g1, g2, bool(c[0])))
        near |= bool(nr[0])
    return out, near
