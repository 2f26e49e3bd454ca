"""Build and run tests/chain_report/check_chain_report.cpp (the host program of the contact report
for arms) — TEST INFRASTRUCTURE ONLY, shared by tests/test_chain_report_host.py and
tests/test_gpu_chain_report.py.  The flags are tests/chain_host.py::build's."""
import os
import subprocess

import numpy as np

from tests import chain_host as H

HERE = os.path.dirname(os.path.abspath(__file__))


def build(out, extra=()):
    return subprocess.run([H.hipcc(), "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-mfma",
                           "-I" + H.CSRC, "-I" + os.path.join(H.ROOT, "include"), *extra,
                           os.path.join(HERE, "chain_report", "check_chain_report.cpp"), os.path.join(H.CSRC, "mjcf.cpp"),
                           "-o", out], capture_output=True, text=True)


def chain(exe, xml, D, q, tmp, tag="r"):
    """chain_build + the report routines over the poses q [N, D]: rc / err, info, pairs
    [(g1, g2, moving1, moving2, margin)], statics [(g1, g2, margin, contact, deep)], contact and deep
    [N, P] uint8, contact_only [N, P] (the report without deep), first [N] int32 (the lowest column
    in contact, -1: none)"""
    q = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1, D))
    pin, pout = os.path.join(str(tmp), tag + ".q"), os.path.join(str(tmp), tag + ".out")
    q.tofile(pin)
    o = H._run([exe, "chain", xml, str(D), pin, pout])
    o["pairs"], o["statics"] = [], []
    for w in o["lines"]:
        if w[0] == "info":
            o["info"] = dict(zip(("n_driven_bodies", "n_geoms", "n_moving_geoms", "n_static_geoms", "n_pairs",
                                  "n_static_pairs", "static_contacts"), (int(x) for x in w[1:])))
        elif w[0] == "pair":
            o["pairs"].append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), float(w[5])))
        elif w[0] == "spair":
            o["statics"].append((int(w[1]), int(w[2]), float(w[3]), int(w[4]), int(w[5])))
    if o["rc"] == 0 and "info" in o:
        P = o["info"]["n_pairs"]
        for k in ("contact", "deep", "contact_only"):
            o[k] = np.fromfile(pout + "." + k, np.uint8).reshape(len(q), P)
        o["first"] = np.fromfile(pout + ".first", np.int32)
        assert len(o["first"]) == len(q)
    return o


def twin(exe, xml, qpos, tmp, tag="t"):
    """the free-body twin through the scene builder's env-env path: pairs [(g1, g2)], contact and
    deep [N, P] uint8"""
    qpos = np.ascontiguousarray(np.asarray(qpos, np.float64))
    pin, pout = os.path.join(str(tmp), tag + ".q"), os.path.join(str(tmp), tag + ".out")
    qpos.tofile(pin)
    o = H._run([exe, "twin", xml, pin, pout])
    o["pairs"] = [(int(w[1]), int(w[2])) for w in o["lines"] if w[0] == "spair"]
    if o["rc"] == 0:
        for k in ("contact", "deep"):
            o[k] = np.fromfile(pout + "." + k, np.uint8).reshape(len(qpos), len(o["pairs"]))
    return o


def first_of(contact):
    """the lowest nonzero column of each row of contact [..., P], -1 for a row of zeros"""
    hit = np.asarray(contact) > 0
    if hit.shape[-1] == 0:
        return np.full(hit.shape[:-1], -1, np.int32)
    return np.where(hit.any(-1), hit.argmax(-1), -1).astype(np.int32)


def path_first(contact):
    """[B, 2] int32 (waypoint, pair) of the dense path report contact [B, W + 1, P]"""
    col = first_of(contact)                       # [B, W + 1]
    touched = col >= 0
    wp = np.where(touched.any(1), touched.argmax(1), -1).astype(np.int32)
    pair = np.where(wp >= 0, col[np.arange(len(col)), np.maximum(wp, 0)], -1).astype(np.int32)
    return np.stack([wp, pair], 1)
