"""First timings of the contact report for arms (recorded, not barred: first numbers, untuned).

HIP-event medians, each call timed alone after warm-up of its shape, on the 7-joint capsule arm of
tests/chain_scenes.py (capsule_arm_world(7, 11): 7 driven bodies, 52 pairs):
  pair_contacts   sspp_chain_pair_contacts on 4096 x 128 poses, with and without deep
  path_contacts   sspp_chain_path_contacts on 4096 splines x 128 check points (129 waypoints each)
  first_contacts  sspp_chain_first_contacts on the same splines
and, for scale, in the same run on the same inputs: Chain.contacts' launch on the poses and
Chain.score_ctrl on the splines (tools/chain_timing.py's rows).  The dense report runs both
colliders of every pair of every pose and writes 27 MB per count; Chain.contacts and score_ctrl stop
a pose at its first contact (score_ctrl a whole candidate), and so does first_contacts.

    python tools/chain_report_timing.py [--reps 200] > profiles/chain_report_timing.txt
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
    ap.add_argument("--reps", type=int, default=200)
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
    P = info["n_pairs"]
    N = B * W
    q = torch.from_numpy(Wd.arm_poses(D, N, 1, 2.0)).cuda()
    hit = torch.empty((N,), dtype=torch.uint8, device="cuda")
    pc = torch.empty((N, P), dtype=torch.uint8, device="cuda")
    pd = torch.empty((N, P), dtype=torch.uint8, device="cuda")
    rows.append(("pair_contacts with deep, %d poses x %d pairs" % (N, P), timed(
        torch, lambda: _lib.check(L.sspp_chain_pair_contacts(ch.handle, vp(q), N, vp(pc), vp(pd), st())), a.reps)))
    rows.append(("pair_contacts without deep, same poses", timed(
        torch, lambda: _lib.check(L.sspp_chain_pair_contacts(ch.handle, vp(q), N, vp(pc), None, st())), a.reps)))
    rows.append(("for scale: Chain.contacts' launch, same poses", timed(
        torch, lambda: _lib.check(L.sspp_chain_contacts(ch.handle, vp(q), N, vp(hit), st())), a.reps)))
    touching = float(hit.float().mean())
    pairs_per_touching = float((pc > 0).sum()) / max(1.0, float(hit.sum()))
    del pc, pd
    # tools/chain_timing.py's splines: around the linear path between two free poses of a pool, of
    # a few such queries the one whose candidates are nearest to half feasible
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
    dk = knots.ctypes.data_as(C.POINTER(C.c_double))
    n = int(ctrl.shape[1])
    wc = torch.empty((B, W + 1, P), dtype=torch.uint8, device="cuda")
    wd = torch.empty((B, W + 1, P), dtype=torch.uint8, device="cuda")
    first = torch.empty((B, 2), dtype=torch.int32, device="cuda")
    rows.append(("path_contacts with deep, %d splines x %d waypoints x %d pairs" % (B, W + 1, P), timed(
        torch, lambda: _lib.check(L.sspp_chain_path_contacts(ch.handle, dk, 3, vp(ctrl), B, n, W, vp(wc), vp(wd), st())),
        a.reps)))
    rows.append(("path_contacts without deep, same splines", timed(
        torch, lambda: _lib.check(L.sspp_chain_path_contacts(ch.handle, dk, 3, vp(ctrl), B, n, W, vp(wc), None, st())),
        a.reps)))
    rows.append(("first_contacts, same splines", timed(
        torch, lambda: _lib.check(L.sspp_chain_first_contacts(ch.handle, dk, 3, vp(ctrl), B, n, W, vp(first), st())),
        a.reps)))
    rows.append(("for scale: Chain.score_ctrl, same splines (arc lengths, feasibility, argmin)", timed(
        torch, lambda: ch.score_ctrl(knots, 3, ctrl, W, 0, arc, feas, best), a.reps)))
    feasible = float(feas.float().mean())
    fw = first[:, 0]
    late = float((fw >= 64).float().mean())
    assert bool(((fw < 0) == (feas != 0)).all()) or ch.info()["static_contacts"] > 0

    print("# microseconds (HIP events), %s, %d repetitions per row after 3 warm-up launches" % (torch.cuda.get_device_name(0), a.reps))
    print("# first numbers, untuned: nothing was tuned against them")
    print("# the arm: %d driven bodies, %d moving and %d static geoms, %d pairs" %
          (info["n_driven_bodies"], info["n_moving_geoms"], info["n_static_geoms"], P))
    print("%-84s %12s %12s" % ("", "median", "p90"))
    for name, (med, p90) in rows:
        print("%-84s %12.1f %12.1f" % (name, med, p90))
    print("# poses in contact: %.3f (%.2f pairs per touching pose); feasible splines: %.3f; first contact in the second or"
          " third pass (waypoint >= 64): %.3f of the splines" % (touching, pairs_per_touching, feasible, late))


if __name__ == "__main__":
    main()
