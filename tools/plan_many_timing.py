"""Time per query of SamplingPathPlanner7.plan_many against a loop of plan() calls.

Robocrane at the drop-in's shape (4096 samples x 128 check points, 10 init points).  For Q in
1, 4, 16, 64: the median wall time of plan_many over Q queries, and of Q plan() calls in a loop,
same process, same planner object, same queries; both divided by Q.  Warm-up first (job creation,
the hit-order pre-pass, buffers), then five repeats with the two forms interleaved.

    python tools/plan_many_timing.py [--iters 30] > profiles/plan_many_timing.txt
"""
import argparse
import contextlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, W, N = 4096, 128, 10
QS = (1, 4, 16, 64)
REPEATS = 5


@contextlib.contextmanager
def quiet():
    """plan() prints one line per call (as the reference does); keep it out of the table."""
    sys.stdout.flush()
    saved = os.dup(1)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(null)
        os.close(saved)


def queries(Q):
    quat = [0.707, 0, 0, 0.707]
    starts = np.array([[0.5, 0.15 + 0.001 * k, 0.136 + 0.001 * k] + quat for k in range(Q)])
    ends = np.array([[0.5, -0.05 - 0.001 * k, 0.136 + 0.001 * k] + quat for k in range(Q)])
    return starts, ends


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30, help="timed calls per repeat and form")
    a = ap.parse_args()
    import sspp_amd as S
    from sspp import _sspp
    planner = _sspp.SamplingPathPlanner7(os.path.join(S.SCENE_DIR, "robocrane.xml"))
    sigma, limits = 0.08, np.ones(7)
    kw = dict(sample_count=B, check_points=W, init_points=N)

    def many(starts, ends):
        planner.plan_many(starts, ends, sigma, limits, **kw)

    def loop(starts, ends):
        for s, e in zip(starts, ends):
            planner.plan(s, e, sigma, limits, **kw)

    def timed(f, starts, ends, iters):
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            f(starts, ends)
            ts.append(time.perf_counter() - t0)
        return ts

    rows = []
    with quiet():
        for Q in QS:
            starts, ends = queries(Q)
            iters = max(3, a.iters // max(1, Q // 4))
            for f in (many, loop):      # warm-up: jobs, tables, buffers, the pre-pass lands
                timed(f, starts, ends, 3)
            time.sleep(0.2)
            for f in (many, loop):
                timed(f, starts, ends, 2)
            tm, tl = [], []
            for _ in range(REPEATS):    # interleaved
                tm.append(statistics.median(timed(many, starts, ends, iters)) / Q * 1e6)
                tl.append(statistics.median(timed(loop, starts, ends, iters)) / Q * 1e6)
            rows.append((Q, iters, tm, tl))
    print("# microseconds per query, robocrane %d x %d, %d init points; median of `iters` calls per repeat," % (B, W, N))
    print("# %d repeats interleaved (plan_many, then the plan() loop); [min .. max] of the repeats' medians" % REPEATS)
    print("%4s %6s  %-34s %-34s %s" % ("Q", "iters", "plan_many", "loop of plan()", "ratio of medians"))
    for Q, iters, tm, tl in rows:
        f = lambda t: "%8.2f [%8.2f .. %8.2f]" % (statistics.median(t), min(t), max(t))  # noqa: E731
        print("%4d %6d  %-34s %-34s %.2f" % (Q, iters, f(tm), f(tl), statistics.median(tl) / statistics.median(tm)))


if __name__ == "__main__":
    main()
