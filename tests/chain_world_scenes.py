"""Worlds for arms: the test cells and their worlds — TEST INFRASTRUCTURE ONLY.

Built from tests/chain_scenes.py's helpers.  A cell is dict(world, D, nq, names); a world of a cell is
dict(qpos=[nq] or None, poses=[(body name, pos, quat), ...]): the values sspp_chain_set_qpos takes,
then the sspp_chain_set_body_pose calls in order.  Quaternions are given as they are passed in, not
normalised: the product normalises them once, as the loader normalises those of a rewritten MJCF, and
norm_world does the same here (the loader's operations on Python floats: the same IEEE results).

  cell   the 7-joint capsule arm planned with dof = 5: joints 5 (a slide with ref != 0) and 6 (a hinge)
         are frozen joints on driven bodies; a static door (a box on a hinge on a jointless body), a
         free block (a sphere, qpos 8..14), a jointless pillar, and obstacles().  nq = 15
  base   the 3-joint arm on a free base, dof = 9: the base and two joints are driven, the third joint
         (a slide, qpos 9) is frozen, and the free joint of a second free body (qpos 10..16) follows.
         With dof = 3 the pose rule cuts the base: its quaternion comes from the world.  nq = 17
  full   the 3-joint arm with nq == D == 3: worlds are accepted and change nothing
"""
import copy
import math

import numpy as np

from tests import chain_scenes as W


def normq(q):
    """sspp::loader_normq on Python floats"""
    q = [float(x) for x in q]
    s = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    n = math.sqrt(s)
    return [x / n for x in q] if n > 0 else [1.0, 0.0, 0.0, 0.0]


def norm_world(qpos, free_adrs):
    """qpos with the quaternion of every free joint (at free_adrs) normalised as the product does"""
    q = [float(x) for x in qpos]
    for a in free_adrs:
        q[a + 3:a + 7] = normq(q[a + 3:a + 7])
    return np.array(q)


BLOCK_R = 0.05
BLOCK_REST = (0.5, -0.3, 0.045)  # 5 mm into the floor: a static contact
BLOCK_UP = (0.5, -0.3, 0.4)


def cell():
    w = W.capsule_arm_world(7, 11)
    door = dict(name="door", pos=(0, 0, 0), joints=[dict(type="hinge", axis=(0, 0, 1), pos=(0, -0.15, 0), name="door_hinge")],
                geoms=[dict(name="door_g", type=W.BOX, size=(0.02, 0.15, 0.25))], children=[])
    w["bodies"].append(dict(name="frame", pos=(1.0, -0.4, 0.6), children=[door]))
    w["bodies"].append(dict(name="block", pos=BLOCK_REST, free=True, children=[],
                            geoms=[dict(name="block_g", type=W.SPHERE, size=(BLOCK_R, 0, 0))]))
    w["bodies"].append(dict(name="pillar", pos=(-0.3, -0.4, 0.0), children=[],
                            geoms=[dict(name="pillar_g", type=W.CAPSULE, size=(0.04, 0.3, 0), pos=(0, 0, 0.35))]))
    return dict(world=w, D=5, nq=15, door=7, block=8, frozen=(5, 6), free=(8,))


def base():
    w = W.capsule_arm_world(3, 21, free_base=True)
    w["bodies"].append(dict(name="puck", pos=(0.4, 0.3, 0.5), free=True, children=[],
                            geoms=[dict(name="puck_g", type=W.SPHERE, size=(0.06, 0, 0))]))
    return dict(world=w, D=9, nq=17, block=10, cut_D=3, free=(0, 10))


def full():
    return dict(world=W.capsule_arm_world(3, 21), D=3, nq=3, free=())


def cell_worlds(qpos0):
    """four worlds of the cell: the model's own; frozen joints, door and block moved; another set with
    the block beside the arm; the second again with four bodies re-posed (a static jointless body, the
    door's jointless parent, the arm's base and the last link: bodies inside the driven chain)"""
    q0 = np.asarray(qpos0, float)
    w1 = q0.copy()
    w1[5], w1[6], w1[7] = q0[5] - 0.05, 0.5, 1.1
    w1[8:15] = list(BLOCK_UP) + [0.9, 0.1, -0.3, 0.2]
    w2 = q0.copy()
    w2[5], w2[6], w2[7] = q0[5] - 0.06, -1.3, -0.7
    w2[8:15] = [0.2, 0.25, 0.6] + [0.3, -0.5, 0.4, 0.7]
    poses = [("pillar", (-0.35, 0.2, 0.05), [0.95, 0.1, 0.2, 0.0]),
             ("frame", (0.95, -0.45, 0.55), [0.98, 0.0, 0.0, 0.2]),
             ("link0", (0.05, -0.04, 0.33), [0.97, 0.1, -0.1, 0.15]),
             ("link6", (0.01, 0.02, 0.31), [0.8, 0.3, 0.2, -0.4])]
    return [dict(qpos=None, poses=[]), dict(qpos=w1, poses=[]), dict(qpos=w2, poses=[]), dict(qpos=w1, poses=poses)]


def base_worlds(qpos0):
    """the model's own world, and one with the base's quaternion (read only where dof cuts the base),
    the frozen slide and the puck moved"""
    q0 = np.asarray(qpos0, float)
    w1 = q0.copy()
    w1[3:7] = [0.7, -0.2, 0.6, 0.1]
    w1[9] = q0[9] + 0.11
    w1[10:17] = [0.1, -0.2, 0.55] + [0.5, 0.5, -0.5, 0.5]
    return [dict(qpos=None, poses=[]), dict(qpos=w1, poses=[])]


def with_world(world, name_pose):
    """the cell's dict with bodies re-posed (a free body's pose is its qpos0 in the MJCF): the world
    a rewritten MJCF expresses"""
    w = copy.deepcopy(world)

    def walk(b):
        if b["name"] in name_pose:
            b["pos"], b["quat"] = tuple(name_pose[b["name"]][0]), tuple(name_pose[b["name"]][1])
        for c in b.get("children", ()):
            walk(c)

    for b in w["bodies"]:
        walk(b)
    return w


def cell_poses(D, n, seed):
    """n poses of the cell's driven joints, tests/chain_scenes.py's spread"""
    return W.arm_poses(D, n, seed, 2.0)
