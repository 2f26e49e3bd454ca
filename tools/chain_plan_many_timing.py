"""Time per query of Chain.plan_many against a loop of sspp_chain_plan_host calls (first numbers,
recorded, not barred: nothing is tuned against them).

The 7-joint capsule arm of tools/chain_timing.py (tests/chain_scenes.py capsule_arm_world(7, 11)),
distinct queries between free poses of one pool.  Two shapes: the one the reference's users plan an
arm with (100 samples x 100 check points, 7 init points) and the drop-in's large one (4096 x 128,
10 init points).  For Q in 1, 4, 16, 64: the median wall time of one Chain.plan_many over Q queries,
and of Q sspp_chain_plan_host calls in a loop (with ctrl_out, as the drop-in planner of an arm calls
it: the winner's control points come from there), same process, same chain, same queries; both
divided by Q.  Warm-up first (the chain's job of the shape, buffers), then five repeats with the two
forms interleaved.

    python tools/chain_plan_many_timing.py [--iters 30] > profiles/chain_plan_many_timing.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 7
SHAPES = ((100, 100, 7), (4096, 128, 10))  # sample_count, check_points, init_points
QS = (1, 4, 16, 64)
REPEATS = 5
SIGMA = 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30, help="timed calls per repeat and form")
    a = ap.parse_args()
    import torch

    import sspp_amd as S
    from sspp_amd import _lib
    from tests import chain_scenes as Wd
    assert torch.cuda.is_available(), "the timings need a GPU"
    L = _lib.lib()
    with tempfile.TemporaryDirectory() as tmp:
        xml = os.path.join(tmp, "arm7.xml")
        with open(xml, "w") as f:
            f.write(Wd.mjcf(Wd.capsule_arm_world(7, 11)))
        model = S.Model(xml, joints=True)
    ch = S.Chain(model, D)
    info = ch.info()
    pool = torch.from_numpy(Wd.arm_poses(D, 2000, 1, 2.0)).cuda() * 0.6
    free = pool[ch.contacts(pool) == 0].cpu().numpy()
    assert len(free) >= max(QS) + 4, "too few free poses in the pool"
    starts = np.ascontiguousarray(free[:max(QS)])
    ends = np.ascontiguousarray(np.array([free[np.argsort(np.abs(free - s).max(1))[3]] for s in starts]))
    limits = np.pi * np.ones(D)
    seeds = [S.DEFAULT_SEED + k for k in range(max(QS))]
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731

    def timed(f, iters):
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return ts

    print("# microseconds per query (wall clock), %s; the arm: %d driven bodies, %d pairs; sigma %g" %
          (torch.cuda.get_device_name(0), info["n_driven_bodies"], info["n_pairs"], SIGMA))
    print("# first numbers, untuned: nothing was tuned against them")
    print("# median of `iters` calls per repeat, %d repeats interleaved (plan_many, then the loop);" % REPEATS)
    print("# [min .. max] of the repeats' medians")
    for B, W, n in SHAPES:
        knots, ctrl = np.zeros(n + 4), np.zeros((B, n, D))
        feas, arc, best = np.zeros(B, np.uint8), np.zeros(B), _lib.Best()
        rows = []
        for Q in QS:
            s, e, sd = starts[:Q], ends[:Q], seeds[:Q]
            winners = []

            def many():
                out = ch.plan_many(s, e, SIGMA, limits, B, W, n, seeds=sd)
                winners[:] = [b[1] for b in out["best"]]

            def loop():
                for k in range(Q):
                    _lib.check(L.sspp_chain_plan_host(ch.handle, dp(s[k]), dp(e[k]), SIGMA, dp(limits), B, W, n, sd[k],
                                                      dp(knots), dp(ctrl), feas.ctypes.data_as(C.POINTER(C.c_uint8)), dp(arc),
                                                      C.byref(best)), "chain plan")

            iters = max(3, a.iters // max(1, Q // 4))
            for f in (many, loop):  # warm-up: the job of the shape, the buffers
                timed(f, 3)
            tm, tl = [], []
            for _ in range(REPEATS):  # interleaved
                tm.append(statistics.median(timed(many, iters)) / Q * 1e6)
                tl.append(statistics.median(timed(loop, iters)) / Q * 1e6)
            rows.append((Q, iters, tm, tl, sum(w >= 0 for w in winners)))
        print("\n## %d samples x %d check points, %d init points" % (B, W, n))
        print("%4s %6s  %-34s %-34s %-16s %s" % ("Q", "iters", "plan_many", "loop of sspp_chain_plan_host", "ratio of medians",
                                                   "queries with a winner"))
        for Q, iters, tm, tl, won in rows:
            f = lambda t: "%8.2f [%8.2f .. %8.2f]" % (statistics.median(t), min(t), max(t))  # noqa: E731
            print("%4d %6d  %-34s %-34s %-16.2f %d" % (Q, iters, f(tm), f(tl), statistics.median(tl) / statistics.median(tm), won))


if __name__ == "__main__":
    main()
