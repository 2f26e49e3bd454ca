"""numpy reference of the contact report for arms — TEST INFRASTRUCTURE ONLY.

Written from the rule (DESIGN.md §5 "Contact report for arms"), sharing no code with the product:
tests/chain_ref.py's forward kinematics and pair table, and per pair the signed distances of the
sphere tests its rule runs (tests/chain_ref.pair_dist: tests/capsule_ref.py's capsule rules plus
plane-sphere, sphere-sphere and sphere-box), nan where a test is not run.  Per pose and pair

    contact = #(d <= margin)        deep = #(d < -1e-3)

over the tests that ran, both 0 for a pair the bounding-sphere cull removes (a zero bounding radius,
a plane's, is never culled).  With the margins >= 0 of every world here a distance below -1e-3 is a
contact, so `deep` is capsule_ref's "a contact and dist < -1e-3".  The parallel capsule-capsule
rule (end +h1, -h1 of capsule 1 against segment 2, then end +h2, -h2 of capsule 2 against segment 1,
until two contacts are found) comes with capsule_ref's run mask: a test past the second contact
is nan here and counts for neither.
"""
import numpy as np

from tests import chain_ref as R

DEEP = -1e-3


def report(m, D, q):
    """(contact [N, P] uint8, deep [N, P] uint8, gap): gap is the least |d - margin| or |d - DEEP|
    over every test that ran on an unculled pair (how far the nearest count is from changing)"""
    _, _, gpos, gmat = R.fk(m, R.full_qpos(m, q))
    mv, _ = R.pairs(m, D)
    N = len(gpos)
    contact, deep = np.zeros((N, len(mv)), np.uint8), np.zeros((N, len(mv)), np.uint8)
    gap = np.inf
    for k, (g1, g2, margin) in enumerate(mv):
        a, b = (g1, g2) if m["geoms"][g1]["type"] <= m["geoms"][g2]["type"] else (g2, g1)
        A, B = m["geoms"][a], m["geoms"][b]
        d = R.pair_dist(A["type"], gpos[:, a], gmat[:, a], A["size"], B["type"], gpos[:, b], gmat[:, b], B["size"], margin)
        keep = np.ones(N, bool)
        ra, rb = R.rbound(A), R.rbound(B)
        if ra > 0 and rb > 0:
            keep = ~(((gpos[:, b] - gpos[:, a]) ** 2).sum(1) > (ra + rb + margin) ** 2)
        with np.errstate(invalid="ignore"):
            c, dp = (d <= margin), (d < DEEP)
        assert not (c & ~keep[:, None]).any()  # (the broadphase is conservative)
        contact[:, k] = (c & keep[:, None]).sum(1)
        deep[:, k] = (dp & keep[:, None]).sum(1)
        ran = d[keep]
        if ran.size and np.isfinite(ran).any():
            gap = min(gap, float(np.nanmin(np.minimum(np.abs(ran - margin), np.abs(ran - DEEP)))))
    return contact, deep, gap

