"""GPU parity at the contact thresholds over the FP32 filter's whole certified envelope: the
scenes of tests/envelope_scenes.py — root coordinates at 7.5 .. 7.99 m and just past 8 m, a partner
centred 15.5 m out (and past 16 m), pair extents S = 2, 4, 7.5 (and past 8), one and two mover
geoms 1.5 m off their root with rotations of their own, and two movers (D = 9) — with poses
+-eps {1e-3 .. 4} and +-{1e-9, 1e-7} m from a threshold, eps the scene table's own 2e-4 max(1, S).

A wrong certain FP32 decision flips a feasibility flag; so does a pose the kernel composes wrongly
in FP32 (the geom's offset and rotation, the mover partner) if the error passes eps.  The bars are
test_gpu_boundary_poses.py's: feasibility and the argmin record equal to the oracle's, arcs within
COST_TOL, and here also the launch with the filter byte-equal to the one without, and the scan the
library reports: fp32-filtered exactly where f32_eps's envelope holds.  That the poses follow the
sign of their offsets, with both outcomes everywhere, is tests/test_envelope_scenes.py's (no GPU).
"""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as O
from tests import boundary_poses as BP
from tests import envelope_scenes as E
from tests import synth_scenes as Y
from tests.test_gpu_boundary_poses import (N_CTRL, SPAN_END, SPAN_START, Bundle, W, assert_parity, candidates,
                                           run_score_ctrl, sampled_around)
from tests.test_gpu_parity import linear_init
from tests.test_gpu_synthetic_scenes import LAUNCH, MIN_EACH, B, oracle_sample_score, steps_case

pytestmark = pytest.mark.gpu

VARIANTS = ("equal", "approach", "mirrored")


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("envelope_scenes"))
    made = {}

    def get(name, margin):
        key = (name, margin)
        if key not in made:
            made[key] = Bundle(root, "env_%s_m%g" % key, E.scene(name, margin), 0, E.DOF[name])
        return made[key]

    return dict(root=root, get=get)


def span(name):
    """The job's own initial spline: across the scene; a second mover stays where its cases park it."""
    tail = np.array(E.M1_POS[:2]) if E.DOF[name] == 9 else np.zeros(0)
    return linear_init(np.concatenate([SPAN_START, tail]), np.concatenate([SPAN_END, tail]), N_CTRL)


def reference(world, b, name, margin, knots, variant):
    """Once per (scene, margin, variant): the candidates and the oracle's scores of them."""
    key = ("ref", variant)
    if key not in b.memo:
        _, cases, P, _ = E.envelope_set(world["root"], name, margin)
        ctrl = candidates(P, variant)
        arc, feas = O.sspp_score(b.r.full, knots, 3, ctrl, W)
        for a in (ctrl, arc, feas):
            a.setflags(write=False)
        # one waypoint decides each candidate (tests/test_envelope_scenes.py: 1 m on nothing touches)
        assert np.array_equal(feas == 0, P["off"] < 0)
        b.memo[key] = (ctrl, arc, feas)
    return b.memo[key]


@pytest.mark.parametrize("nt,g1", LAUNCH)
@pytest.mark.parametrize("name", E.SCENES)
def test_score_ctrl_at_the_envelope(world, name, nt, g1):
    """score_ctrl on every pose of one scene, both margins, the three control-row variants, pair
    orders 0 and 2, with the filter and without: oracle parity for both, the two byte-equal, and
    the reported scan fp32-filtered exactly where the table lies inside the envelope."""
    knots, ctrl0 = span(name)
    limits = np.ones(E.DOF[name])
    for margin in E.MARGINS:
        b = world["get"](name, margin)
        want = Y.expected_scan(b.r.ref, E.DOF[name])
        assert want == E.SCAN[name]
        for variant in VARIANTS:
            ctrl, arc_o, feas_o = reference(world, b, name, margin, knots, variant)
            for order in (0, 2):
                got = {}
                for f32 in (1, 0):
                    job, arc, feas, best = run_score_ctrl(b, knots, ctrl0, ctrl, nt, g1, f32, order, limits)
                    assert_parity(arc, feas, best, arc_o, feas_o)
                    cfg = job.config()
                    assert cfg["scan"] == (want if f32 else "fp64"), (margin, variant, order, f32)
                    assert cfg["pair_order"] == {0: "scene", 2: "hit"}[order] and not cfg["split"]
                    got[f32] = (arc.tobytes(), feas.tobytes(), best)
                assert got[1] == got[0], (margin, variant, order)


@pytest.mark.parametrize("margin", E.MARGINS)
@pytest.mark.parametrize("name", E.SCENES)
def test_sampled_around_envelope_poses(world, name, margin):
    """sample_score with sigma = 1e-6 around every pose: the kernel's own FP32 copies of the
    sampled control rows feed the scan.  A job's sampled table holds the pairs its candidates can
    reach, and the filter's margin is that table's: a touching pose keeps its target pair, and a
    table that holds a pair past a cut-off is scanned in FP64."""
    b = world["get"](name, margin)
    _, cases, P, _ = E.envelope_set(world["root"], name, margin)
    dof = E.DOF[name]
    jobs = sampled_around(b, P, lambda knots, ctrl: O.sspp_score(b.r.full, knots, 3, ctrl, W), dof, np.ones(dof))
    over = {"far_partner_out": "wall", "large_over": "wall"}.get(name)
    for i in range(0, len(jobs), 3):
        cfg = jobs[i].config()
        touching = P["off"][i] <= -BP.FLOOR
        if touching:
            assert cfg["sampled_pairs"] >= 1, i
        if over is None:
            assert cfg["scan"] == ("fp32-filtered" if cfg["sampled_pairs"] else "fp64"), i
        elif touching and cases[P["case"][i]]["target"] == over:
            assert cfg["scan"] == "fp64", i


def test_split_launch_sees_an_offset_geom(world):
    """offset_one through the step executor: 8 steps x 2048 candidates in one split launch (twice),
    sampled with sigma = the table's eps around one grazing pose (1.1 eps clear) of the offset,
    rotated geom on the tilted box, so that the queue consumers' own FP32 scan composes that
    geom's pose on both sides of the band.  Every step equals the oracle, the launch ran split and no survivor was lost."""
    import sspp_amd as S
    b = world["get"]("offset_one", 0.0)
    _, cases, P, eps = E.envelope_set(world["root"], "offset_one", 0.0)
    i = next(i for i, k in enumerate(P["case"]) if cases[k]["feature"] == "tilted" and cases[k]["family"] == "c"
             and P["off"][i] == eps * 1.1)
    q = P["q"][i]
    side = SimpleNamespace(scene=b.scene, oscene=b.r.full, memo=b.memo)
    job, knots, ctrl0 = steps_case(side, q, q, eps, np.ones(7), 8, split=1)
    assert job.get_option(S._lib.OPT_LAST_SPLIT) == 1 and job.get_option(S._lib.OPT_SPLIT_LOST) == 0
    cfg = job.config()
    assert cfg["scan"] == "fp32-filtered" and cfg["sampled_pairs"] >= 1
    _, _, feas_o = oracle_sample_score(side, knots, ctrl0, eps, np.ones(7), 5 * B, B)
    assert MIN_EACH <= int(feas_o.sum()) <= B - MIN_EACH
