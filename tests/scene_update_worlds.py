"""The re-posed worlds of the scene-update tests (tests/test_scene_update_host.py,
tests/test_gpu_scene_update.py): each world is a dict {body name: (pos, quat or None)} applied three
ways — to an MJCF file (a fresh product object's input), to the oracle's model dict, and through
the product's update calls.  pos is the body's `pos` attribute (world position of a top-level
body), quat its `quat` (None: the file's).
"""
import os
import re

import numpy as np

from tests.conftest import SCENES

ROBOCRANE = os.path.join(SCENES, "robocrane.xml")
STACKING = os.path.join(SCENES, "stacking.xml")
GRIPPER = "gripper_collision_with_block/"
IDENT = (1.0, 0.0, 0.0, 0.0)

# robocrane.xml: A the file as it is; N the gripper next to the brick stack;
# F the gripper resting in the floor; W2 / W1 a jointless wall body moved
WALL1_POS, WALL2_POS = (0.5, 0.05, 0.116), (0.5, 0.05, 0.156)   # the file's
CRANE = {
    "A": {},
    "N": {GRIPPER: ((0.5, 0.05, 0.40), IDENT)},
    "F": {GRIPPER: ((2.0, 2.2, 0.0), IDENT)},
    "W2": {"blockwall2": ((0.5, 0.05 + 0.3, 0.156), None)},
    "W1": {"blockwall1": ((0.5, 0.05, 0.116 + 0.08), None)},
}
GRIPPER_A = ((2.0, 2.2, 0.5), IDENT)
# entries inside a scene's own driven window are no obstacles but the defaults of the mover's
# undriven components: D3 turns block_green (SamplingPathPlanner3 drives its position only: the
# quaternion is the default), D9 lifts and turns block_orange (SamplingPathPlanner9 drives its x, y)
DRIVEN = {
    "D3": {"block_green/": ((0.5, 0.15, 0.116), IDENT)},
    "D9": {"block_orange/": ((0.5, -0.05, 0.30), IDENT)},
}
# stacking.xml: block3 lifted away / block3 pushed into block2
STACK = {
    "A": {},
    "S1": {"block3": ((0.1, 0.0, 0.62), IDENT)},
    "S2": {"block3": ((0.0, 0.15, 0.1), IDENT)},
}
BLOCK3_A = ((-0.205, 0.0, 0.1), IDENT)

START7 = np.array([0.5, 0.168, 0.222, 0.707, 0, 0, 0.707])
END7 = np.array([0.5, -0.062, 0.222, 0.707, 0, 0, 0.707])


def _fmt(v):
    return " ".join(repr(float(x)) for x in v)


def write_xml(src, dst, edits):
    """src with every edited body's pos (and quat) attribute replaced; returns dst."""
    text = open(src).read()
    for name, (pos, quat) in edits.items():
        m = re.search(r'<body name="%s"[^>]*>' % re.escape(name), text)
        assert m, name
        tag = m.group(0)
        new = re.sub(r' pos="[^"]*"', "", tag)
        if quat is not None:
            new = re.sub(r' quat="[^"]*"', "", new)
        attrs = ' pos="%s"' % _fmt(pos) + ('' if quat is None else ' quat="%s"' % _fmt(quat))
        new = new.replace('<body name="%s"' % name, '<body name="%s"%s' % (name, attrs), 1)
        text = text.replace(tag, new, 1)
    with open(dst, "w") as f:
        f.write(text)
    return str(dst)


def edit_model(md, edits):
    """A copy of the oracle's model dict (oracle/mjcf_ref.load) with the edits applied: body_pos /
    body_quat, and qpos0 for a free body; quaternions normalised as the loaders do (q / |q|)."""
    md = dict(md)
    for k in ("body_pos", "body_quat", "qpos0"):
        md[k] = np.array(md[k], np.float64, copy=True)
    for name, (pos, quat) in edits.items():
        b = md["body_names"].index(name)
        md["body_pos"][b] = pos
        if quat is not None:
            q = np.asarray(quat, np.float64)
            md["body_quat"][b] = q / np.sqrt((q * q).sum())
        if md["body_jnt_type"][b] == 0:
            a = int(md["body_qpos_adr"][b])
            md["qpos0"][a:a + 3] = md["body_pos"][b]
            md["qpos0"][a + 3:a + 7] = md["body_quat"][b]
    return md


def qpos_for(md, edits):
    """The whole qpos of the edited world (free bodies only), unnormalised as a caller passes it."""
    q = np.array(md["qpos0"], np.float64, copy=True)
    for name, (pos, quat) in edits.items():
        b = md["body_names"].index(name)
        assert md["body_jnt_type"][b] == 0, name
        a = int(md["body_qpos_adr"][b])
        q[a:a + 3] = pos
        if quat is not None:
            q[a + 3:a + 7] = quat
    return q
