"""What the query sets of tests/chain_query_cases.py hold, decided on the host without a GPU by the
stand-alone program tests/chain/check_chain.cpp (the routines the chain kernels loop over).

sspp_sample_ctrl_host samples through a device job, so the candidates of a mixed
query are not available here: tests/test_gpu_chain_queries.py asserts the mixed counts from this
program's decisions before it compares anything with the device.  Here:
  blocked  waypoint 0 of every candidate is the first control point of a clamped spline, which the
           sampler leaves alone (the touching pose up to the interpolation's rounding): the program
           finds that control point in contact, so no candidate of the query is feasible whatever
           the noise
  tie      sigma = 0 leaves every candidate the initial spline, and the program finds every one of
           its waypoints free: every candidate is feasible
These assertions are about the test sets and hold with or without the query calls; the last test
checks that the two calls are declared, bound and exported.
"""
import numpy as np
import pytest

import sspp_amd as S
from tests import chain_host as H
from tests import chain_query_cases as QC
from tests import chain_scenes as W
from tests import test_gpu_chain as G


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chain_queries") / "check_chain")
    r = H.build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize("arm", sorted(QC.SETS))
def test_blocked_and_tie_queries(exe, tmp_path, arm):
    c = QC.SETS[arm]
    nj, seed, fb = G.ARMS[arm]
    xml = H.write_xml(tmp_path, arm, W.mjcf(G.arm_world(nj, seed, fb)))
    for n in sorted({c["n"], 4, 8}):
        qs = QC.make(S, exe, tmp_path, xml, arm, n=n)
        assert qs["kinds"] == list(QC.ORDER) and QC.BLOCKED in qs["kinds"] and QC.TIE in qs["kinds"]
        assert len(set(qs["sigma"])) > 2 and len(set(qs["seeds"].tolist())) == len(qs["seeds"])
        assert len({tuple(row) for row in qs["limits"]}) == len(qs["limits"])
        for q, kind in enumerate(qs["kinds"]):
            init = qs["init"][q]
            if kind == QC.BLOCKED:
                assert 0 < qs["sigma"][q] < 0.05
                # the clamped spline's first control point is the touching pose up to the interpolation's
                # rounding, and the spline's value at u = 0: the program decides that very pose
                assert np.abs(init[0] - qs["starts"][q]).max() < 1e-14
                assert S.spline_eval(qs["knots"], c["degree"], init, 0.0).tobytes() == init[0].tobytes()
                hit = H.chain(exe, xml, c["D"], init[:1], tmp_path, tag="blocked")["hit"]
                assert hit.tolist() == [1]
            elif kind == QC.TIE:
                assert qs["sigma"][q] == 0.0
                assert np.abs(init).max() < qs["limits"][q].min()  # (nothing for the sampler to clip)
                for Wc in (40, 64, 65):
                    feas, _ = G.host_feasible(S, exe, tmp_path, xml, c["D"], qs["knots"], c["degree"], init[None], Wc, "tie")
                    assert feas.tolist() == [True], (arm, n, Wc)
            else:
                assert qs["sigma"][q] >= 0.05


def test_query_calls_are_declared_and_bound():
    """the two query calls of a chain: declared in include/sspp_hip.h, bound in sspp_amd/_lib.py with
    the header's argument counts, exported by the library, and reachable as Chain methods"""
    from sspp_amd import _lib
    declared = _lib.declared_symbols()
    for name, nargs in (("sspp_chain_sample_score_queries", 18), ("sspp_chain_plan_many_host", 17)):
        assert name in declared and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib(), name), name
    assert callable(getattr(S.Chain, "sample_score_queries", None)) and callable(getattr(S.Chain, "plan_many", None))
