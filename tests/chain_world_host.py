"""Build and run tests/chain_world/check_world.cpp (the host program of the worlds of arms) — TEST
INFRASTRUCTURE ONLY, shared by tests/test_chain_world_host.py and tests/test_gpu_chain_world.py.  The
flags are tests/chain_host.py::build's."""
import os
import subprocess

import numpy as np

from tests import chain_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


def build(out, extra=()):
    return subprocess.run([H.hipcc(), "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-mfma",
                           "-I" + H.CSRC, "-I" + os.path.join(H.ROOT, "include"), *extra,
                           os.path.join(HERE, "chain_world", "check_world.cpp"), os.path.join(H.CSRC, "mjcf.cpp"),
                           "-o", out], capture_output=True, text=True)


def _nums(v):
    return " ".join(repr(float(x)) for x in np.asarray(v, float).reshape(-1))


def op_qpos(qpos, raw=False):
    return "%s %d %s" % ("rawqpos" if raw else "qpos", len(qpos), _nums(qpos))


def op_body(body, pos, quat, raw=False):
    return "%s %d %s %s" % ("rawbody" if raw else "body", body, _nums(pos), _nums(quat))


def world_ops(body_names, world):
    """the product ops of a world of tests/chain_world_scenes.py: set_qpos, then the set_body_pose calls"""
    ops = [] if world["qpos"] is None else [op_qpos(world["qpos"])]
    return ops + [op_body(body_names.index(name), pos, quat) for name, pos, quat in world["poses"]]


def run(exe, xml, D, ops, q, tmp, count_static=0, tag="w"):
    """the chain after ops over the poses q [N, D]: rc / err, ops [(rc, epoch, hash, err)], info, pairs,
    statics [(g1, g2, margin, contact, deep)], epoch, hash, qpos, tables (bytes), fk [N, ngeom, 12],
    hit [N], contact / deep [N, P], first [N]"""
    q = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1, D))
    base = os.path.join(str(tmp), tag)
    q.tofile(base + ".q")
    with open(base + ".ops", "w") as f:
        f.write("\n".join(ops) + "\n")
    o = H._run([exe, "run", xml, str(D), str(int(count_static)), base + ".ops", base + ".q", base + ".out"])
    o["pairs"], o["statics"], o["ops"] = [], [], []
    for w in o["lines"]:
        if w[0] == "info":
            o["info"] = dict(zip(("n_driven_bodies", "n_geoms", "n_moving_geoms", "n_static_geoms", "n_pairs",
                                  "n_static_pairs", "static_contacts"), (int(x) for x in w[1:])))
        elif w[0] == "pair":
            o["pairs"].append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), float(w[5])))
        elif w[0] == "spair":
            o["statics"].append((int(w[1]), int(w[2]), float(w[3]), int(w[4]), int(w[5])))
        elif w[0] == "op":
            o["ops"].append([int(w[1]), int(w[2]), int(w[3]), ""])
        elif w[0] == "err" and o["ops"]:
            o["ops"][-1][3] = " ".join(w[1:])
        elif w[0] == "epoch":
            o["epoch"] = int(w[1])
        elif w[0] == "hash":
            o["hash"] = int(w[1])
        elif w[0] == "qpos":
            o["qpos"] = np.array([float(x) for x in w[1:]])
    if o["rc"] == 0 and "info" in o:
        ng, P = o["info"]["n_geoms"], o["info"]["n_pairs"]
        with open(base + ".out.tables", "rb") as f:
            o["tables"] = f.read()
        o["fk"] = np.fromfile(base + ".out.fk", np.float64).reshape(len(q), ng, 12)
        o["hit"] = np.fromfile(base + ".out.hit", np.uint8)
        for k in ("contact", "deep"):
            o[k] = np.fromfile(base + ".out." + k, np.uint8).reshape(len(q), P)
        o["first"] = np.fromfile(base + ".out.first", np.int32)
        assert len(o["hit"]) == len(q) == len(o["first"])
    return o
