"""Time to plan in a changed world: re-posing the scene in place against rebuilding everything.

Robocrane at the drop-in's shape (4096 samples x 128 check points, 10 init points); the world
alternates between the file's (the gripper parked at (2, 2.2, 0.5)) and the gripper next to the
brick stack at (0.5, 0.05, 0.40), so every repetition changes the pair tables.
  (a) update:  SamplingPathPlanner7.set_qpos(qpos), then plan() on the same planner.
  (b) rebuild: the MJCF written with the new pose, SamplingPathPlanner7(xml), its first plan()
      — the only path before scene updates existed (this half runs without them too).
Median and p90 of the wall time over `--reps` repetitions after warm-up, in microseconds.

    python tools/scene_update_timing.py [--reps 200] > profiles/scene_update_timing.txt
"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_many_timing import quiet  # noqa: E402

B, W, N = 4096, 128, 10
GRIPPER = "gripper_collision_with_block/"
POSES = ((2.0, 2.2, 0.5), (0.5, 0.05, 0.40))


def write_xml(src, dst, pos):
    text = open(src).read()
    tag = re.search(r'<body name="%s"[^>]*>' % re.escape(GRIPPER), text).group(0)
    new = re.sub(r' pos="[^"]*"', ' pos="%r %r %r"' % pos, tag)
    with open(dst, "w") as f:
        f.write(text.replace(tag, new, 1))


def stats(ts):
    ts = sorted(ts)
    return statistics.median(ts) * 1e6, ts[min(len(ts) - 1, int(0.9 * len(ts)))] * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    import sspp_amd as S
    from sspp import _sspp
    src = os.path.join(S.SCENE_DIR, "robocrane.xml")
    quat = [0.707, 0, 0, 0.707]
    start, end = np.array([0.5, 0.168, 0.222] + quat), np.array([0.5, -0.062, 0.222] + quat)
    sigma, limits = 0.1, np.ones(7)
    kw = dict(sample_count=B, check_points=W, init_points=N)
    rows = []
    with quiet(), tempfile.TemporaryDirectory() as d:
        xml = os.path.join(d, "world.xml")

        def rebuild(i):
            t0 = time.perf_counter()
            write_xml(src, xml, POSES[i & 1])
            p = _sspp.SamplingPathPlanner7(xml)
            p.plan(start, end, sigma, limits, **kw)
            return time.perf_counter() - t0

        for i in range(10):          # warm-up: the process's streams, code objects, allocator
            rebuild(i)
        rows.append(("(b) rebuild: write MJCF + new planner + first plan()", stats([rebuild(i) for i in range(a.reps)])))

        planner = _sspp.SamplingPathPlanner7(src)
        if hasattr(planner, "set_qpos"):
            planner.plan(start, end, sigma, limits, **kw)
            qpos = [np.array(planner.get_qpos()) for _ in POSES]
            for q, pos in zip(qpos, POSES):
                q[21:24] = pos

            def update(i):
                t0 = time.perf_counter()
                planner.set_qpos(qpos[i & 1])
                t1 = time.perf_counter()
                planner.plan(start, end, sigma, limits, **kw)
                return t1 - t0, time.perf_counter() - t0

            for i in range(10):
                update(i + 1)
            ts = [update(i + 1) for i in range(a.reps)]
            rows.append(("(a) update: set_qpos + plan()", stats([t[1] for t in ts])))
            rows.append(("    of which set_qpos", stats([t[0] for t in ts])))
    print("# microseconds, robocrane %d x %d, %d init points; %d repetitions after warm-up, the world alternating" % (B, W, N, a.reps))
    print("%-56s %12s %12s" % ("", "median", "p90"))
    for name, (med, p90) in rows:
        print("%-56s %12.1f %12.1f" % (name, med, p90))
    if len(rows) > 1:
        print("# rebuild / update (medians): %.1f" % (rows[0][1][0] / rows[1][1][0]))


if __name__ == "__main__":
    main()
