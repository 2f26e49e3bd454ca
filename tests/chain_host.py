"""Build and run tests/chain/check_chain.cpp (the articulated movers' host program) — TEST
INFRASTRUCTURE ONLY, shared by tests/test_chain_host.py and tests/test_gpu_chain.py."""
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sspp_amd", "csrc")
SAN_FLAGS = ["-g", "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"]


def hipcc():
    h = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert h, "the host build needs hipcc"
    return h


def build(out, extra=()):
    return subprocess.run([hipcc(), "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-mfma",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), *extra,
                           os.path.join(HERE, "chain", "check_chain.cpp"), os.path.join(CSRC, "mjcf.cpp"), "-o", out],
                          capture_output=True, text=True)


def sanitizer_probe(d):
    """None when a one-line program builds and runs with SAN_FLAGS, else why not"""
    probe = os.path.join(str(d), "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    exe = os.path.join(str(d), "probe")
    p = subprocess.run([hipcc(), "-x", "hip", "--offload-host-only", *SAN_FLAGS, probe, "-o", exe],
                       capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 0:
        return (p.stderr.strip().splitlines() or ["probe failed"])[-1][:200]
    return None


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = dict(stderr=r.stderr, rc=None, err="", lines=[ln.split() for ln in r.stdout.splitlines() if ln.strip()])
    for ln in r.stdout.splitlines():
        if ln.startswith("rc "):
            out["rc"] = int(ln.split()[1])
        elif ln.startswith("err "):
            out["err"] = ln[4:]
    return out


def load(exe, xml, joints=True):
    """the loader's result: rc / err, and on success nq, qpos0, bodies [(jnt_type, qpos_adr, jnt_adr,
    jnt_num)], joints [(type, body, adr, axis, pos, name)]"""
    o = _run([exe, "load", "joints" if joints else "strict", xml])
    o["bodies"], o["joints"] = [], []
    for w in o["lines"]:
        if w[0] == "nq":
            o["nq"] = int(w[1])
        elif w[0] == "qpos0":
            o["qpos0"] = np.array([float(x) for x in w[1:]])
        elif w[0] == "body":
            o["bodies"].append(tuple(int(x) for x in w[2:6]))
        elif w[0] == "jnt":
            o["joints"].append((int(w[1]), int(w[2]), int(w[3]), np.array([float(x) for x in w[4:7]]),
                                np.array([float(x) for x in w[7:10]]), w[10] if len(w) > 10 else ""))
    return o


def chain(exe, xml, D, q, tmp, count_static=0, tag="c"):
    """chain_build + the per-pose routines over the poses q [N, D]: rc / err, info, pairs
    [(g1, g2, moving1, moving2, margin)], fk [N, ngeom, 12] (position, then the matrix), hit [N]"""
    q = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1, D))
    pin, pout = os.path.join(str(tmp), tag + ".q"), os.path.join(str(tmp), tag + ".out")
    q.tofile(pin)
    o = _run([exe, "chain", xml, str(D), str(int(count_static)), pin, pout])
    o["pairs"] = []
    for w in o["lines"]:
        if w[0] == "info":
            o["info"] = dict(zip(("n_driven_bodies", "n_geoms", "n_moving_geoms", "n_static_geoms", "n_pairs",
                                  "n_static_pairs", "static_contacts"), (int(x) for x in w[1:])))
        elif w[0] == "pair":
            o["pairs"].append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), float(w[5])))
    if o["rc"] == 0 and "info" in o:
        ng = o["info"]["n_geoms"]
        o["fk"] = np.fromfile(pout + ".fk", np.float64).reshape(len(q), ng, 12)
        o["hit"] = np.fromfile(pout + ".hit", np.uint8)
        assert len(o["hit"]) == len(q)
    return o


def twin(exe, xml, qpos, tmp, tag="t"):
    """the free-body twin through the scene builder's env-env path: pairs [(g1, g2)], contact [N, P]"""
    qpos = np.ascontiguousarray(np.asarray(qpos, np.float64))
    pin, pout = os.path.join(str(tmp), tag + ".q"), os.path.join(str(tmp), tag + ".out")
    qpos.tofile(pin)
    o = _run([exe, "twin", xml, pin, pout])
    o["pairs"] = [(int(w[1]), int(w[2])) for w in o["lines"] if w[0] == "spair"]
    if o["rc"] == 0:
        o["contact"] = np.fromfile(pout + ".contact", np.uint8).reshape(len(qpos), len(o["pairs"]))
    return o


def write_xml(tmp, name, text):
    p = os.path.join(str(tmp), name + ".xml")
    with open(p, "w") as f:
        f.write(text)
    return p
