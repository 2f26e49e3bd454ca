"""First timings of the contact report (recorded, not barred: nothing was tuned against them).

HIP-event medians, each launch timed alone after warm-up of its shape:
  (a) pose form:  Scene.contacts on 65536 poses of robocrane's gripper as a TaskSpacePlanner body
      (48 pairs), contact + deep and contact only;
  (b) path form:  SsppJob.path_contacts on 4096 splines x 128 check points on robocrane (dof 7),
      contact + deep and contact only; beside it score_ctrl over the same splines for scale;
  (c) TaskSpacePlanner path form: TspJob.path_contacts on 4096 via sets x 128 check points on the
      gripper scene; beside it score_vias over the same via sets.
The report tests every pair at every waypoint of every path and writes every count; the scoring
kernels stop a candidate at its first contact and cull pairs per candidate, so the report is
expected to take longer.

    python tools/contact_report_timing.py [--reps 30] > profiles/contact_report_timing.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIPPER = "gripper_collision_with_block/"
N_POSES, B, W = 65536, 4096, 128


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
    import ctypes as C

    import torch

    import sspp_amd as S
    from oracle import oracle as O
    from sspp_amd import _lib
    assert torch.cuda.is_available(), "the timings need a GPU"
    L = _lib.lib()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    path = os.path.join(S.SCENE_DIR, "robocrane.xml")
    model = S.Model(path)
    rows = []

    # (a) pose form
    tscene = S.Scene(model, 1, GRIPPER)
    P = tscene.info()["n_pairs"]
    rng = np.random.default_rng(1)
    q = np.stack([rng.uniform(0.15, 0.8, N_POSES), rng.uniform(-0.25, 0.35, N_POSES), rng.uniform(0.0, 0.4, N_POSES),
                  rng.uniform(-1.6, 1.6, N_POSES)], 1)
    dq = torch.from_numpy(q).cuda()
    c = torch.empty((N_POSES, P), dtype=torch.uint8, device="cuda")
    d = torch.empty_like(c)
    for deep in (d, None):
        fn = lambda deep=deep: _lib.check(L.sspp_scene_contacts(tscene.handle, vp(dq), N_POSES, vp(c), vp(deep), st()))  # noqa: E731
        rows.append(("(a) pose form, %d poses x %d pairs, %s" % (N_POSES, P, "contact + deep" if deep is not None else "contact only"),
                     timed(torch, fn, a.reps)))
    touching = float((c > 0).any(1).float().mean())

    # (b) SamplingPathPlanner path form
    scene = S.Scene(model, 0, 7)
    P7 = scene.info()["n_pairs"]
    start = np.array([0.5, 0.168, 0.222, 0.707, 0, 0, 0.707])
    end = np.array([0.5, -0.062, 0.222, 0.707, 0, 0, 0.707])
    u = np.array([i / 9 for i in range(10)])
    knots, ctrl0 = S.interpolate(np.array([(1 - t) * start + t * end for t in u]), 3, u)
    job = S.SsppJob(scene, knots, 3, ctrl0, 0.1, np.ones(7), W, max_batch=B)
    ctrl = torch.from_numpy(O.sample_sspp(ctrl0, 3, 0.1, np.ones(7), 0x5EED, 0, B)).cuda()
    pc = torch.empty((B, W + 1, P7), dtype=torch.uint8, device="cuda")
    pd = torch.empty_like(pc)
    for deep in (pd, None):
        fn = lambda deep=deep: _lib.check(L.sspp_job_path_contacts(job._h, vp(ctrl), B, vp(pc), vp(deep), st()))  # noqa: E731
        rows.append(("(b) path form, %d x %d waypoints x %d pairs, %s" % (B, W + 1, P7, "contact + deep" if deep is not None else "contact only"),
                     timed(torch, fn, a.reps)))
    o = job.alloc(B)
    rows.append(("    score_ctrl over the same splines", timed(torch, lambda: job.score_ctrl(ctrl, 0, o["arc"], o["feasible"], o["best"]), a.reps)))
    hit7 = float(pc.view(B, -1).any(1).float().mean())

    # (c) TaskSpacePlanner path form
    ts, te = np.array([0.2, 0.05, 0.2, 0.0]), np.array([0.85, 0.05, 0.2, 0.8])
    lo, hi = np.array([0.0, -0.45, 0.0, -1.6]), np.array([1.0, 0.55, 0.6, 1.6])
    mean = np.stack([ts + (te - ts) * (k + 1) / 3 for k in range(2)])
    sigma = np.full((2, 4), 0.15)
    tjob = S.TspJob(tscene, ts, te, 2, W, mean=mean, sigma=sigma, lo=lo, hi=hi, max_batch=B)
    vias = torch.from_numpy(O.sample_tsp(mean, sigma, lo, hi, 0.0, 0x5EED, 0, B)).cuda()
    tc = torch.empty((B, W, P), dtype=torch.uint8, device="cuda")
    td = torch.empty_like(tc)
    fn = lambda: _lib.check(L.sspp_job_path_contacts(tjob._h, vp(vias), B, vp(tc), vp(td), st()))  # noqa: E731
    rows.append(("(c) TaskSpacePlanner path form, %d x %d waypoints x %d pairs, contact + deep" % (B, W, P), timed(torch, fn, a.reps)))
    to = tjob.alloc(B)
    rows.append(("    score_vias over the same via sets",
                 timed(torch, lambda: tjob.score_vias(vias, 0, to["L"], to["Cnf"], to["Cwf"], to["status"], to["cost"], to["best"]), a.reps)))
    deep_t = float(td.view(B, -1).any(1).float().mean())

    print("# microseconds (HIP events), %s, %d repetitions per row after 3 warm-up launches" % (torch.cuda.get_device_name(0), a.reps))
    print("# first numbers for these kernels: nothing was tuned against them")
    print("%-84s %12s %12s" % ("", "median", "p90"))
    for name, (med, p90) in rows:
        print("%-84s %12.1f %12.1f" % (name, med, p90))
    print("# poses with a contact (a): %.3f; splines with a contact (b): %.3f; via sets with a deep contact (c): %.3f"
          % (touching, hit7, deep_t))


if __name__ == "__main__":
    main()
