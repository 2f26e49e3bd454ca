"""CPU checks of tests/dof_degree_cases.py: every scene case is non-vacuous under the oracle
alone, the case lists reach the tails and sizes they name, and arc_ref is a sound reference.
tests/test_gpu_dof_degree.py runs the same cases on the device (sspp_sample_ctrl_host among
them: it samples through a device job, so it cannot run here)."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import dof_degree_cases as C


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("dof_degree_cases")


def sampled(root, D, p, n, sigma, sampler=0, first=C.FIRST, B=C.B, W=C.W, seed=C.SEED, scene=None):
    """The oracle's feasibility of the initial spline and of B sampled candidates."""
    knots, ctrl0 = C.init_spline(D, p, n)
    _, _, lim = C.ends(D)
    osc = C.oracle_scene(root, scene or C.scene_name(D), D)
    _, f0 = O.sspp_score(osc, knots, p, ctrl0[None], W)
    ctrl = O.sample_sspp(ctrl0, p, sigma, lim, seed, first, B, sampler=sampler)
    _, feas = O.sspp_score(osc, knots, p, ctrl, W)
    return bool(f0[0]), feas


def assert_mixed(feas):
    nf = int(feas.sum())
    assert C.MIN_EACH <= nf <= len(feas) - C.MIN_EACH, nf


# ------------------------------------------------------------------ non-vacuity
def test_window_quaternion_is_not_the_identity(root):
    from oracle import mjcf_ref
    ref = mjcf_ref.load(C.write_scene(root, "window"))
    np.testing.assert_allclose(ref["qpos0"][3:7], C.Q0, rtol=0, atol=1e-15)
    assert abs(C.Q0[0]) < 0.95 and len(ref["qpos0"]) == 7
    one = mjcf_ref.load(C.write_scene(root, "window_one"))
    assert len(one["geom_type"]) == len(ref["geom_type"]) - 1


@pytest.mark.parametrize("D,p,n", C.matrix_cases())
def test_matrix_case_is_mixed(root, D, p, n):
    f0, feas = sampled(root, D, p, n, C.sigma_for(D))
    assert f0  # the initial spline is free
    assert_mixed(feas)


def test_matrix_covers_every_instantiation_and_an_odd_npert():
    cases = C.matrix_cases()
    assert {(D, p) for D, p, _ in cases} == {(D, p) for D in C.DOFS for p in C.DEGREES}
    rows = {n - 2 * p for _, p, n in cases}
    assert {1, 2} <= rows and max(rows) >= 4
    assert any(C.npert(D, p, n) % 2 == 1 for D, p, n in cases)
    assert C.FIRST >= 2 ** 32


@pytest.mark.parametrize("D,p,n", C.FP32_CASES)
def test_fp32_case_is_mixed(root, D, p, n):
    f0, feas = sampled(root, D, p, n, C.sigma_for(D), sampler=O.SAMPLER_FP32)
    assert f0
    assert_mixed(feas)


def test_fp32_cases_cover_the_quad_tails():
    assert [C.npert(*c) for c in C.FP32_CASES] == [1, 3, 6, 7, 18]
    assert {C.npert(*c) % 4 for c in C.FP32_CASES} == {1, 2, 3}


def test_nopert_cases_perturb_nothing(root):
    for D, p, n, with_scene in C.nopert_cases():
        assert C.npert(D, p, n) == 0
        knots, ctrl0 = C.init_spline(D, p, n)
        _, _, lim = C.ends(D)
        ctrl = O.sample_sspp(ctrl0, p, C.NOPERT_SIGMA, lim, C.SEED, C.NOPERT_FIRST, 4)
        assert all(np.array_equal(c, ctrl0) for c in ctrl)
        if with_scene:  # feasible by construction
            _, f = O.sspp_score(C.oracle_scene(root, C.scene_name(D), D), knots, p, ctrl0[None], C.W)
            assert f[0] == 1
    first, last = C.NOPERT_FIRST, C.NOPERT_FIRST + C.NOPERT_B - 1
    assert first >> 32 != last >> 32


@pytest.mark.parametrize("D,p", C.W1_CASES)
def test_w1_case_is_mixed(root, D, p):
    assert_mixed(C.w1_expected(root, D, p)[3])


@pytest.mark.parametrize("N", [3, 6, 9])
def test_dropin_case_is_mixed(root, N):
    f0, feas = sampled(root, N, 3, C.DROPIN["init_points"], C.sigma_for(N), first=0, seed=C.DROPIN_SEED,
                       B=C.DROPIN["sample_count"], W=C.DROPIN["check_points"])
    assert f0
    assert_mixed(feas)
    assert C.DROPIN["init_points"] - 2 * 3 == 3  # three perturbed rows


def test_knot_cases_cover_what_they_name():
    cases = C.knot_cases()
    assert {(D, p) for D, p, *_ in cases} == {(D, p) for D in C.DOFS for p in C.DEGREES}
    for p in C.DEGREES:
        mine = [c for c in cases if c[1] == p]
        assert {c[4] for c in mine} == set(C.W_LIST) | {16, 17}
        assert {c[2] for c in mine} == {p + 1, p + 2, 2 * p + 1, 13}
        assert {c[3] for c in mine} == set(C.KNOT_KINDS)
        assert {c[4] for c in mine if c[3] == "grid"} == {16, 17}
    for D, p, n, kind, W in cases:
        knots, ctrl = C.knot_case_data(D, p, n, kind, W)
        inner = knots[p + 1:n]
        assert len(knots) == n + p + 1 and (np.diff(knots) >= 0).all()
        assert (knots[:p + 1] == 0).all() and (knots[n:] == 1).all() and ((inner > 0) & (inner < 1)).all()
        if kind == "double":
            assert inner[0] == inner[1]
        if kind == "grid" and len(inner):
            # every interior knot is a collision parameter i / W (W = 16) or an arc parameter
            # i / (W - 1) (W = 17), as the doubles the scorers form
            grid = [i / W for i in range(W + 1)] if W == 16 else [i / (W - 1) for i in range(W)]
            assert set(inner) <= set(grid)


# ------------------------------------------------------------------ arc_ref is a sound reference
def test_arc_ref_matches_the_reference_robot_path():
    """The reference's own BSplines chord sum of its saved robot path (D = 9, degree 2)."""
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "robot_path.json")))
    got = C.arc_ref(np.array(d["knots"]), 2, np.array(d["ctrl"]), d["W"])
    assert abs(float(got) - d["arc_length"]) <= 1e-15 * d["arc_length"]


def test_arc_ref_basis_is_a_partition_of_unity():
    """At every parameter the (d) cases use — u = 1 and u equal to a knot among them — the basis
    is non-negative and sums to 1."""
    at_knot = 0
    for D, p, n, kind, W in C.knot_cases():
        if D != C.DOFS[0]:  # the basis does not depend on D
            continue
        knots, _ = C.knot_case_data(D, p, n, kind, W)
        u = C.arc_params(W)
        N = C.basis_matrix(knots, p, u)
        assert N.shape == (W, n) and (N >= 0).all()
        assert float(np.abs(N.sum(axis=1) - 1).max()) <= 4 * np.finfo(np.longdouble).eps
        assert u[-1] == 1.0 and N[-1, -1] == 1 and N[0, 0] == 1
        at_knot += int(np.isin(u[1:-1], knots).sum())
        Nk = C.basis_matrix(knots, p, knots)
        assert float(np.abs(Nk.sum(axis=1) - 1).max()) <= 4 * np.finfo(np.longdouble).eps
    assert at_knot > 0


def test_oracle_against_arc_ref():
    """The oracle's largest relative deviation from arc_ref over the (d) cases: the figure
    DESIGN.md §2 records (6.2e-16 with an 80-bit long double) and the device's bar against arc_ref rests on."""
    worst = C.oracle_vs_ref()
    print("oracle vs arc_ref, max relative deviation over %d cases: %.3e -> device bar %.3e"
          % (len(C.knot_cases()), worst, C.ref_bar(worst)))
    # a canonical-order sum of at most 1024 chords of 13-term double dot products cannot lose
    # more than a few ulp to the long-double evaluation
    assert worst <= 32 * np.finfo(np.float64).eps
    assert C.ref_bar(worst) == 1e-12
