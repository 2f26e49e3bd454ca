"""First timings of the articulated movers' kernels (recorded, not barred: first numbers, untuned).

HIP-event medians, each call timed alone after warm-up of its shape, on the 7-joint capsule arm of
tests/chain_scenes.py (capsule_arm_world(7, 11): 7 driven bodies, 52 pairs):
  fk          Chain.fk's launch on 4096 x 128 poses
  contacts    Chain.contacts' launch on the same poses
  score_ctrl  Chain.score_ctrl on 4096 splines x 128 check points (the scene-less job's arc
              lengths, the feasibility kernel, the argmin)
and, for scale, the existing SsppJob.score_ctrl on robocrane.xml (dof 7, free bodies) at the same
shape.  The chain's kernel runs FK of every driven body at every waypoint until a candidate's first
contact; k_sspp_c2f culls pairs per candidate, filters in FP32 and scans coarse to fine.

    python tools/chain_timing.py [--reps 30] > profiles/chain_timing.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, W, D = 4096, 128, 7


def timed(torch, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return statistics.median(ms) * 1e3, ms[min(len(ms) - 1, int(0.9 * len(ms)))] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch

    import sspp_amd as S
    from oracle import oracle as O
    from sspp_amd import _lib
    from tests import chain_scenes as Wd
    assert torch.cuda.is_available(), "the timings need a GPU"
    L = _lib.lib()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    rows = []

    with tempfile.TemporaryDirectory() as tmp:
        xml = os.path.join(tmp, "arm7.xml")
        with open(xml, "w") as f:
            f.write(Wd.mjcf(Wd.capsule_arm_world(7, 11)))
        model = S.Model(xml, joints=True)
    ch = S.Chain(model, D)
    info = ch.info()
    N = B * W
    q = torch.from_numpy(Wd.arm_poses(D, N, 1, 2.0)).cuda()
    gpos = torch.empty((N, info["n_geoms"], 3), dtype=torch.float64, device="cuda")
    gmat = torch.empty((N, info["n_geoms"], 9), dtype=torch.float64, device="cuda")
    hit = torch.empty((N,), dtype=torch.uint8, device="cuda")
    rows.append(("fk, %d poses, %d geoms" % (N, info["n_geoms"]),
                 timed(torch, lambda: _lib.check(L.sspp_chain_fk(ch.handle, vp(q), N, vp(gpos), vp(gmat), st())), a.reps)))
    rows.append(("contacts, %d poses x %d pairs" % (N, info["n_pairs"]),
                 timed(torch, lambda: _lib.check(L.sspp_chain_contacts(ch.handle, vp(q), N, vp(hit), st())), a.reps)))
    touching = float(hit.float().mean())
    # splines around the linear path between two free poses of a pool: of a few such queries, the
    # one whose candidates are nearest to half feasible (a planner's working point)
    pool = q[:400] * 0.6
    free = pool[ch.contacts(pool) == 0].cpu().numpy()
    u = np.array([i / 9 for i in range(10)])
    arc = torch.empty((B,), dtype=torch.float64, device="cuda")
    feas = torch.empty((B,), dtype=torch.uint8, device="cuda")
    best = S.best_tensor()
    pick = None
    for k in range(min(12, len(free))):
        start = free[k]
        end = free[np.argsort(np.abs(free - start).max(1))[3]]
        knots, ctrl0 = S.interpolate(np.array([(1 - t) * start + t * end for t in u]), 3, u)
        ctrl = torch.from_numpy(O.sample_sspp(ctrl0, 3, 0.05, np.pi * np.ones(D), 0x5EED, 0, B)).cuda()
        ch.score_ctrl(knots, 3, ctrl, W, 0, arc, feas, best)
        torch.cuda.synchronize()
        frac = float(feas.float().mean())
        if pick is None or abs(frac - 0.5) < abs(pick[0] - 0.5):
            pick = (frac, knots, ctrl)
    _, knots, ctrl = pick
    rows.append(("score_ctrl, %d splines x %d check points x %d pairs" % (B, W, info["n_pairs"]),
                 timed(torch, lambda: ch.score_ctrl(knots, 3, ctrl, W, 0, arc, feas, best), a.reps)))
    feasible = float(feas.float().mean())

    path = os.path.join(S.SCENE_DIR, "robocrane.xml")
    scene = S.Scene(S.Model(path), 0, 7)
    s0 = np.array([0.5, 0.168, 0.222, 0.707, 0, 0, 0.707])
    s1 = np.array([0.5, -0.062, 0.222, 0.707, 0, 0, 0.707])
    rk, rc0 = S.interpolate(np.array([(1 - t) * s0 + t * s1 for t in u]), 3, u)
    job = S.SsppJob(scene, rk, 3, rc0, 0.1, np.ones(7), W, max_batch=B)
    rctrl = torch.from_numpy(O.sample_sspp(rc0, 3, 0.1, np.ones(7), 0x5EED, 0, B)).cuda()
    o = job.alloc(B)
    rows.append(("for scale: SsppJob.score_ctrl on robocrane.xml, %d x %d, %d pairs" % (B, W, scene.info()["n_pairs"]),
                 timed(torch, lambda: job.score_ctrl(rctrl, 0, o["arc"], o["feasible"], o["best"]), a.reps)))
    rfeas = float(o["feasible"].float().mean())

    print("# microseconds (HIP events), %s, %d repetitions per row after 3 warm-up launches" % (torch.cuda.get_device_name(0), a.reps))
    print("# first numbers, untuned: nothing was tuned against them")
    print("# the arm: %d driven bodies, %d moving and %d static geoms, %d pairs" %
          (info["n_driven_bodies"], info["n_moving_geoms"], info["n_static_geoms"], info["n_pairs"]))
    print("%-84s %12s %12s" % ("", "median", "p90"))
    for name, (med, p90) in rows:
        print("%-84s %12.1f %12.1f" % (name, med, p90))
    print("# poses in contact: %.3f; feasible splines on the arm: %.3f, on robocrane: %.3f" % (touching, feasible, rfeas))


if __name__ == "__main__":
    main()
