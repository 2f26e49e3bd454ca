"""Time of re-posing an arm's world in place and of a world per query (first numbers, recorded, not
barred: nothing is tuned against them).

The 7-joint capsule arm of tools/chain_timing.py (tests/chain_scenes.py capsule_arm_world(7, 11)),
dof = 7, with a free block (a sphere, qpos 7..13) beside it: a world is the block's pose.  Medians of
`iters` calls per repeat, five repeats with the compared forms interleaved, wall clock.
  1. Chain.set_qpos alone.
  2. Chain.set_qpos + sspp_chain_plan_host, against the sequence the parent commit needs for a new
     world: write the MJCF, Model, Chain, its first sspp_chain_plan_host.  Two shapes: 100 samples x
     100 check points (7 init points) and 4096 x 128 (10 init points).
  3. Chain.plan_many(worlds=) over Q in 4, 16, 64 queries with a world each, per query, against the
     loop of set_qpos + sspp_chain_plan_host per query, and against Chain.plan_many without worlds
     on the same queries (all in one world: the price of the indexed tables).

    python tools/chain_world_timing.py [--iters 20] > profiles/chain_world_timing.txt
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
QS = (4, 16, 64)
REPEATS = 5
SIGMA = 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="timed calls per repeat and form")
    a = ap.parse_args()
    import torch

    import sspp_amd as S
    from sspp_amd import _lib
    from tests import chain_scenes as Wd
    assert torch.cuda.is_available(), "the timings need a GPU"
    L = _lib.lib()
    world = Wd.capsule_arm_world(7, 11)
    world["bodies"].append(dict(name="block", pos=(0.5, -0.3, 0.4), free=True, children=[],
                                geoms=[dict(name="block_g", type=Wd.SPHERE, size=(0.05, 0, 0))]))
    tmp = tempfile.mkdtemp()

    def write(block_pos, name):
        world["bodies"][-1]["pos"] = tuple(block_pos)
        path = os.path.join(tmp, name)
        with open(path, "w") as f:
            f.write(Wd.mjcf(world))
        return path

    model = S.Model(write((0.5, -0.3, 0.4), "arm7.xml"), joints=True)
    ch = S.Chain(model, D)
    info = ch.info()
    q0 = ch.get_qpos()
    pool = torch.from_numpy(Wd.arm_poses(D, 2000, 1, 2.0)).cuda() * 0.6
    free = pool[ch.contacts(pool) == 0].cpu().numpy()
    assert len(free) >= max(QS) + 4, "too few free poses in the pool"
    starts = np.ascontiguousarray(free[:max(QS)])
    ends = np.ascontiguousarray(np.array([free[np.argsort(np.abs(free - s).max(1))[3]] for s in starts]))
    limits = np.pi * np.ones(D)
    seeds = [S.DEFAULT_SEED + k for k in range(max(QS))]
    worlds = np.tile(q0, (max(QS), 1))
    worlds[:, 7] += 0.01 * np.arange(max(QS))  # the block at Q places
    worlds[:, 9] += 0.005 * np.arange(max(QS))
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731

    def timed(f, iters):
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return ts

    fmt = lambda t: "%9.2f [%9.2f .. %9.2f]" % (statistics.median(t), min(t), max(t))  # noqa: E731
    print("# microseconds (wall clock), %s; the arm: %d driven bodies, %d pairs, %d static pairs; sigma %g" %
          (torch.cuda.get_device_name(0), info["n_driven_bodies"], info["n_pairs"], info["n_static_pairs"], SIGMA))
    print("# first numbers, untuned: nothing was tuned against them")
    print("# median of `iters` calls per repeat, %d repeats interleaved; [min .. max] of the repeats' medians" % REPEATS)

    flip = [0]

    def repose():
        flip[0] ^= 1
        ch.set_qpos(worlds[1 + flip[0]])

    timed(repose, 3)
    t = [statistics.median(timed(repose, a.iters * 5)) * 1e6 for _ in range(REPEATS)]
    print("\n## 1. Chain.set_qpos alone\n%s" % fmt(t))

    print("\n## 2. a new world, then one plan: in place / a new MJCF, Model and Chain (the parent commit's way)")
    print("%-24s %-36s %-36s %s" % ("shape", "set_qpos + plan_host", "MJCF + Model + Chain + first plan", "ratio of medians"))
    for B, W, n in SHAPES:
        knots, ctrl = np.zeros(n + 4), np.zeros((B, n, D))
        feas, arc, best = np.zeros(B, np.uint8), np.zeros(B), _lib.Best()

        def plan(c, k=0):
            _lib.check(L.sspp_chain_plan_host(c.handle, dp(starts[k]), dp(ends[k]), SIGMA, dp(limits), B, W, n, seeds[k],
                                              dp(knots), dp(ctrl), feas.ctypes.data_as(C.POINTER(C.c_uint8)), dp(arc),
                                              C.byref(best)), "chain plan")

        def in_place():
            repose()
            plan(ch)

        def rebuilt():
            flip[0] ^= 1
            w = worlds[1 + flip[0]]
            c2 = S.Chain(S.Model(write(w[7:10], "next.xml"), joints=True), D)
            plan(c2)

        timed(in_place, 3)
        timed(rebuilt, 2)
        ti, tr = [], []
        iters = max(3, a.iters // (1 if B < 1000 else 4))
        for _ in range(REPEATS):
            ti.append(statistics.median(timed(in_place, iters)) * 1e6)
            tr.append(statistics.median(timed(rebuilt, iters)) * 1e6)
        print("%-24s %-36s %-36s %.2f" % ("%d x %d, %d init" % (B, W, n), fmt(ti), fmt(tr),
                                          statistics.median(tr) / statistics.median(ti)))

    print("\n## 3. a world per query, microseconds per query")
    for B, W, n in SHAPES:
        knots, ctrl = np.zeros(n + 4), np.zeros((B, n, D))
        feas, arc, best = np.zeros(B, np.uint8), np.zeros(B), _lib.Best()
        print("\n### %d samples x %d check points, %d init points" % (B, W, n))
        print("%4s %6s  %-36s %-36s %-36s %-10s %s" % ("Q", "iters", "plan_many(worlds)", "loop of set_qpos + plan_host",
                                                      "plan_many, one world", "loop/worlds", "worlds/plain"))
        for Q in QS:
            s, e, sd, w = starts[:Q], ends[:Q], seeds[:Q], np.ascontiguousarray(worlds[:Q])

            def many_worlds():
                ch.plan_many(s, e, SIGMA, limits, B, W, n, seeds=sd, worlds=w)

            def many_plain():
                ch.plan_many(s, e, SIGMA, limits, B, W, n, seeds=sd)

            def loop():
                for k in range(Q):
                    ch.set_qpos(w[k])
                    _lib.check(L.sspp_chain_plan_host(ch.handle, dp(s[k]), dp(e[k]), SIGMA, dp(limits), B, W, n, sd[k],
                                                      dp(knots), dp(ctrl), feas.ctypes.data_as(C.POINTER(C.c_uint8)), dp(arc),
                                                      C.byref(best)), "chain plan")

            iters = max(3, a.iters // max(1, Q // 4) // (1 if B < 1000 else 2))
            for f in (many_worlds, loop, many_plain):
                timed(f, 2)
            tw, tl, tp = [], [], []
            for _ in range(REPEATS):
                tw.append(statistics.median(timed(many_worlds, iters)) / Q * 1e6)
                tl.append(statistics.median(timed(loop, iters)) / Q * 1e6)
                ch.set_qpos(q0)
                tp.append(statistics.median(timed(many_plain, iters)) / Q * 1e6)
            print("%4d %6d  %-36s %-36s %-36s %-10.2f %.2f" % (Q, iters, fmt(tw), fmt(tl), fmt(tp),
                                                             statistics.median(tl) / statistics.median(tw),
                                                             statistics.median(tw) / statistics.median(tp)))


if __name__ == "__main__":
    main()
