"""Scene re-posing on the host (sspp_scene_build.h), without a GPU: tests/scene_update/check_update.cpp
loads the shipped scenes with the product's MJCF loader and runs the factored table builder — the code
both sspp_scene_create and the scene updates go through — once from the file's poses followed by the
re-pose, and once fresh from a file written with the new poses.  Geoms, pairs, movers and the visit
records must be byte-equal, the static count and cost equal.

Hand-worked values (the worlds are tests/scene_update_worlds.py's):
  * N: the gripper's free joint at (0.5, 0.05, 0.40), identity.  Its body base_mount sits at
    (0, 0, 0.145) turned by quat (0 1 0 0), half a turn about x, so base_mount's geom col_mount at
    (0, 0, 0.016) in that frame lies at (0.5, 0.05, 0.40 + 0.145 - 0.016) = (0.5, 0.05, 0.529).
  * W1: the jointless body blockwall1 from z 0.116 to 0.196 carries its grandchild body
    (pos 0 0 0.02) and that body's box geom: (0.5, 0.05, 0.216).
  * F: the gripper at z 0 rests in the floor: env-env contacts appear (8, cost -1.3453002310774045
    by the CPU oracle: checked against it in tests/test_gpu_scene_update.py; here: > 0 and < 0).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import scene_update_worlds as Wd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sspp_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "the host build needs hipcc"
    out = str(tmp_path_factory.mktemp("scene_update") / "check_update")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "scene_update", "check_update.cpp"), os.path.join(CSRC, "mjcf.cpp"),
                           "-o", out])
    return out


def run(exe, base, fresh, mode, arg, ops):
    args = [exe, base, fresh, str(mode), str(arg)]
    for op in ops:
        args += [str(x) if isinstance(x, str) else repr(float(x)) for x in op]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = dict(rc=[], geom={})
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "rc":
            out["rc"].append(int(w[1]))
        elif w[0] in ("same", "base"):
            out[w[0]] = [int(x) for x in w[1:]]
        elif w[0] == "static":
            out["static"] = (int(w[1]), float(w[2]))
        elif w[0] == "geom":
            out["geom"][w[1]] = np.array([float(x) for x in w[2:5]])
    return out


def body_op(name, pos, quat):
    return ["body", name] + list(pos) + list(quat)


def ops_for(path, edits, whole_qpos):
    """The re-pose as update calls: one set_qpos with the whole vector, or one set_body_pose per body."""
    from oracle import mjcf_ref
    md = mjcf_ref.load(path)
    if whole_qpos:
        return [["qpos"] + list(Wd.qpos_for(md, edits))]
    ops = []
    for name, (pos, quat) in edits.items():
        b = md["body_names"].index(name)
        ops.append(body_op(name, pos, quat if quat is not None else md["body_quat"][b]))
    return ops


CASES = [
    # (file, mode, arg, world, through set_qpos)
    (Wd.ROBOCRANE, 0, 7, "N", True), (Wd.ROBOCRANE, 0, 7, "N", False), (Wd.ROBOCRANE, 0, 7, "F", True),
    (Wd.ROBOCRANE, 0, 7, "W2", False), (Wd.ROBOCRANE, 0, 7, "W1", False), (Wd.ROBOCRANE, 0, 9, "N", True),
    (Wd.ROBOCRANE, 0, 3, "W1", False), (Wd.ROBOCRANE, 1, "block_green/", "N", False),
    (Wd.STACKING, 1, "block1", "S1", True), (Wd.STACKING, 1, "block1", "S2", False), (Wd.STACKING, 1, "block2", "S2", True),
    # entries inside the driven window: the mover's defaults (DMover::qpos0) change, and in a scene
    # that does not drive the body (dof 7 for block_orange) the same edit moves an obstacle
    (Wd.ROBOCRANE, 0, 3, "D3", True), (Wd.ROBOCRANE, 0, 3, "D3", False), (Wd.ROBOCRANE, 0, 9, "D9", True),
    (Wd.ROBOCRANE, 0, 9, "D9", False), (Wd.ROBOCRANE, 0, 7, "D9", True), (Wd.ROBOCRANE, 1, "block_green/", "D3", False),
]


@pytest.mark.parametrize("path,mode,arg,world,whole", CASES)
def test_reposed_tables_equal_fresh_tables(exe, tmp_path, path, mode, arg, world, whole):
    edits = (dict(Wd.CRANE, **Wd.DRIVEN) if path == Wd.ROBOCRANE else Wd.STACK)[world]
    fresh = Wd.write_xml(path, tmp_path / "fresh.xml", edits)
    r = run(exe, path, fresh, mode, arg, ops_for(path, edits, whole))
    assert r["rc"] and all(rc == 0 for rc in r["rc"])
    assert r["same"] == [1, 1, 1, 1, 1], r["same"]
    # not vacuous: the world did change the tables; a driven-window edit changes the movers only
    driven = world in Wd.DRIVEN and not (world == "D9" and arg == 7)
    assert r["base"][:3] == [1, 1, 0] if driven else r["base"][:2] != [1, 1], r["base"]


def test_there_and_back_restores_the_files_tables(exe):
    """N and then the file's pose again: every record is the file's, byte for byte."""
    ops = ops_for(Wd.ROBOCRANE, Wd.CRANE["N"], True) + [body_op(Wd.GRIPPER, *Wd.GRIPPER_A)]
    r = run(exe, Wd.ROBOCRANE, Wd.ROBOCRANE, 0, 7, ops)
    assert r["rc"] == [0, 0] and r["same"] == [1, 1, 1, 1, 1] and r["base"] == [1, 1, 1, 1, 1]


def test_hand_worked_positions(exe):
    n = run(exe, Wd.ROBOCRANE, Wd.ROBOCRANE, 0, 7, ops_for(Wd.ROBOCRANE, Wd.CRANE["N"], True))
    np.testing.assert_allclose(n["geom"][Wd.GRIPPER + "col_mount"], [0.5, 0.05, 0.529], rtol=0, atol=1e-12)
    w1 = run(exe, Wd.ROBOCRANE, Wd.ROBOCRANE, 0, 7, ops_for(Wd.ROBOCRANE, Wd.CRANE["W1"], False))
    np.testing.assert_allclose(w1["geom"]["lego_bricks/block_cyan_geom"], [0.5, 0.05, 0.216], rtol=0, atol=1e-12)
    # the other walls stay where the file puts them
    np.testing.assert_allclose(w1["geom"]["lego_bricks_1/block_magenta_geom"], [0.5, 0.05, 0.176], rtol=0, atol=1e-12)
    a = run(exe, Wd.ROBOCRANE, Wd.ROBOCRANE, 0, 7, [])
    assert a["static"][0] == 0 and a["static"][1] == 0.0
    f = run(exe, Wd.ROBOCRANE, Wd.ROBOCRANE, 0, 7, ops_for(Wd.ROBOCRANE, Wd.CRANE["F"], True))
    assert f["static"][0] > 0 and f["static"][1] < 0.0


def test_quaternions_are_normalised_as_the_loader_does(exe, tmp_path):
    """An unnormalised quaternion through the update equals the same numbers in a file."""
    edits = {Wd.GRIPPER: ((0.5, 0.05, 0.40), (0.707, 0.0, 0.0, 0.707))}
    fresh = Wd.write_xml(Wd.ROBOCRANE, tmp_path / "fresh.xml", edits)
    for whole in (True, False):
        r = run(exe, Wd.ROBOCRANE, fresh, 0, 7, ops_for(Wd.ROBOCRANE, edits, whole))
        assert r["rc"] == [0] and r["same"] == [1, 1, 1, 1, 1]


def test_invalid_updates_change_nothing(exe):
    from oracle import mjcf_ref
    q = np.array(mjcf_ref.load(Wd.ROBOCRANE)["qpos0"])
    zero_quat, nan, inf = q.copy(), q.copy(), q.copy()
    zero_quat[24:28] = 0.0
    nan[21] = np.nan
    inf[3] = np.inf
    bad = [["qpos"] + list(q[:-1]), ["qpos"] + list(q) + [0.0], ["qpos"] + list(zero_quat), ["qpos"] + list(nan),
           ["qpos"] + list(inf),
           body_op("#0", (0, 0, 0), Wd.IDENT), body_op("#-1", (0, 0, 0), Wd.IDENT), body_op("#1000", (0, 0, 0), Wd.IDENT),
           body_op("blockwall1", (0, 0, 0), (0, 0, 0, 0)), body_op("blockwall1", (0, np.nan, 0), Wd.IDENT),
           body_op(Wd.GRIPPER, (0, 0, 0), (np.inf, 0, 0, 0))]
    r = run(exe, Wd.ROBOCRANE, Wd.ROBOCRANE, 0, 7, bad)
    assert r["rc"] == [-1] * len(bad)                    # SSPP_E_INVAL, every one
    assert r["same"] == [1, 1, 1, 1, 1] and r["base"] == [1, 1, 1, 1, 1]
