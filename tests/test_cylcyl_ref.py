"""Cylinder-cylinder narrowphase on the CPU: the numpy reference's accuracy, and a
host build of the device code (tests/cylcyl/check_cylcyl.cpp) against it.

MuJoCo is absent, so the pair is pinned by independent geometry: tests/cylcyl_ref.py maximises
the separation from the support functions by brute force.  Its error E on configurations with an
analytic signed distance is measured here (3.1e-10 at worst, asserted below 5e-10), so decisions
are compared outside a band of 10 x 5e-10 = 5e-9 around each threshold.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cylcyl_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
MARGINS = [0.0, 1e-3, 1e-2]
OFFSETS = [s * m for m in (1e-9, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3) for s in (1.0, -1.0)]
# a rotation in general position, applied to both cylinders: the same signed distance, none of
# the rotations' exact zeros (the identity takes the vertical closed form)
Q = R.rot_axis(np.array([0.6, 0.0, 0.8]), 0.9) @ R.rot_axis(np.array([0.0, 1.0, 0.0]), 0.3)
ROTS = {"identity": np.eye(3), "generic": Q}


def hexrow(*parts):
    return " ".join(float(x).hex() for p in parts for x in np.ravel(p))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """run(cases) -> int array [n, 6]: contacts, deep, deciding stage (contact, deep), the three
    cheap axes' contact and deep decisions; cases = (margin, p1, M1, s1, p2, M2, s2)."""
    d = tmp_path_factory.mktemp("cylcyl_host")
    exe = str(d / "check_cylcyl")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "the host build of the device code needs hipcc"
    subprocess.check_call([hipcc, "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "sspp_amd", "csrc"),
                           os.path.join(HERE, "cylcyl", "check_cylcyl.cpp"), "-o", exe])

    def run(cases):
        path = str(d / "cases.txt")
        with open(path, "w") as f:
            for c in cases:
                f.write(hexrow([c[0]], *c[1:]) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out = np.array([[int(x) for x in line.split()] for line in r.stdout.splitlines()])
        assert out.shape == (len(cases), 6)
        return out

    return run


def case_of(margin, T, M1, R1, H1, M2, R2, H2, rot=np.eye(3)):
    return (margin, np.zeros(3), rot @ M1, [R1, H1, 0.0], rot @ T, rot @ M2, [R2, H2, 0.0])


# ------------------------------------------------------------------ 1. the reference's accuracy
def test_reference_accuracy():
    """E = the largest error of cylcyl_ref.sd on the analytic families (the issue's six and a skew
    rim-rim pair), at rest and in general position, at distances from -3 mm to 3 cm: below E_MAX,
    and the band is 10 E_MAX, at least the 1e-9 floor and at most 1e-6."""
    worst = {}
    for f in R.analytic_families():
        for rn, rot in ROTS.items():
            want = np.array([0.0, 1e-3, 1e-2, 0.03, -1e-3, -3e-3, 1e-9, -1e-9, 1e-3 + 1e-9, 1e-2 - 1e-9, 1e-6, 1e-4])
            if f[0] in R.POSITIVE_ONLY:
                want = want[want > 0]
            P = [R.family_pose(f, R.sd_for_gap(f, w)) for w in want]
            got = R.sd(np.array([rot @ p[0] for p in P]), rot @ P[0][1], P[0][2], P[0][3], rot @ P[0][4], P[0][5], P[0][6])
            worst[(f[0], rn)] = float(np.abs(got - want).max())
    E = max(worst.values())
    print("reference error per family:", worst)
    assert E <= R.E_MAX, worst
    assert R.BAND == max(10 * R.E_MAX, 1e-9) <= 1e-6


def test_scene_shortcut_equals_full_reference():
    """scene_sd's bounds and its cheaper search decide like sd (random pairs around touching, the
    margins and the deep threshold), and the search is reached"""
    rng = np.random.default_rng(3)
    P = [_random_pair(rng) for _ in range(300)]
    arr = lambda k: np.array([p[k] for p in P])  # noqa: E731
    a1, a2 = arr(1)[:, :, 2], arr(5)[:, :, 2]
    full = R.sd(arr(0), a1, arr(2), arr(3), a2, arr(6), arr(7))
    for thr in MARGINS + [R.DEEP]:
        fast, todo = R.scene_sd(arr(0), a1, arr(2), arr(3), a2, arr(6), arr(7), thr)
        assert 0 < todo.sum() < len(P) // 4
        np.testing.assert_array_equal(fast < thr, full < thr)
        np.testing.assert_array_equal(np.abs(fast - thr) <= R.BAND, np.abs(full - thr) <= R.BAND)
        assert np.abs(fast - full)[todo].max() <= R.E_MAX


# ------------------------------------------------------------------ 2. random oriented pairs
def _qmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _random_pair(rng, parallel=False, i=0):
    """(T, M1, R1, H1, _, M2, R2, H2): centre distance spread around touching as
    test_collision_exact._random_pair; parallel: tilts of 1e-9 .. 1e-3 rad, every other pair
    anti-parallel"""
    R1, H1, R2, H2 = rng.uniform(0.02, 0.15, 4)
    q1 = rng.normal(size=4)
    M1 = _qmat(q1 / np.linalg.norm(q1))
    if parallel:
        ax = rng.normal(size=3)
        M2 = R.rot_axis(ax / np.linalg.norm(ax), 10 ** rng.uniform(-9, -3)) @ M1
        if i % 2:
            M2 = M2 @ np.diag([1.0, -1.0, -1.0])
    else:
        q2 = rng.normal(size=4)
        M2 = _qmat(q2 / np.linalg.norm(q2))
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    T = d * rng.uniform(0.3, 1.05) * (math.hypot(R1, H1) + math.hypot(R2, H2))
    return T, M1, R1, H1, None, M2, R2, H2


@pytest.mark.parametrize("parallel", [False, True], ids=["oriented", "nearly_parallel"])
@pytest.mark.parametrize("margin", MARGINS)
def test_random_pairs_match_reference(host_check, margin, parallel):
    """450 pairs: the host build's contact and deep decisions equal the reference's wherever
    |sd - thr| exceeds the band; the three cheap axes alone get some wrong (so the witnesses and
    the search are reached), and the search itself decides some."""
    rng = np.random.default_rng(7 + int(margin * 1000) + (100 if parallel else 0))
    P = [_random_pair(rng, parallel, i) for i in range(450)]
    out = host_check([case_of(margin, p[0], p[1], p[2], p[3], p[5], p[6], p[7]) for p in P])
    arr = lambda k: np.array([p[k] for p in P])  # noqa: E731
    dist = R.sd(arr(0), arr(1)[:, :, 2], arr(2), arr(3), arr(5)[:, :, 2], arr(6), arr(7))
    okc, okd = np.abs(dist - margin) > R.BAND, np.abs(dist - R.DEEP) > R.BAND
    assert okc.sum() > 400 and okd.sum() > 400
    wrong_c = okc & ((out[:, 0] > 0) != (dist < margin))
    wrong_d = okd & ((out[:, 1] > 0) != (dist < R.DEEP))
    assert not wrong_c.any() and not wrong_d.any(), (np.flatnonzero(wrong_c | wrong_d), dist[wrong_c | wrong_d])
    assert (okc & ((out[:, 4] > 0) != (dist < margin))).sum() > 0
    assert parallel or (out[:, 2] == 3).sum() + (out[:, 3] == 3).sum() > 0  # (witnesses settle the parallel set)
    # the cheap-axis bound the reference module offers is the device's (scene_sd relies on neither)
    ch = R.cheap3(arr(0), arr(1)[:, :, 2], arr(2), arr(3), arr(5)[:, :, 2], arr(6), arr(7))
    far = np.abs(ch - margin) > 1e-9
    np.testing.assert_array_equal((out[:, 4] > 0)[far], (ch < margin)[far])


# ------------------------------------------------------------------ 3. crafted threshold poses
@pytest.mark.parametrize("rot", list(ROTS))
@pytest.mark.parametrize("fam", R.analytic_families(), ids=[f[0] for f in R.analytic_families()])
def test_threshold_poses_follow_the_offset(host_check, fam, rot):
    """Each analytic family at sd = thr + offset, offsets +-{1e-9 .. 1e-3}, thr = the margins 0,
    1e-3, 1e-2 (contact iff offset < 0) and the deep threshold (deep iff offset < 0): every
    decision follows the offset's sign down to the project's 1e-9 floor."""
    cases, want_c, want_d = [], [], []
    pos_only = fam[0] in R.POSITIVE_ONLY  # a family whose distance is analytic only when separated
    for mg in MARGINS:
        for off in OFFSETS:
            if pos_only and mg + off <= 0:
                continue
            p = R.family_pose(fam, R.sd_for_gap(fam, mg + off))
            cases.append(case_of(mg, p[0], p[7], p[2], p[3], p[8], p[5], p[6], ROTS[rot]))
            want_c.append(off < 0)
            want_d.append(None)
    for off in ([] if pos_only else OFFSETS):
        p = R.family_pose(fam, R.sd_for_gap(fam, R.DEEP + off))
        cases.append(case_of(0.0, p[0], p[7], p[2], p[3], p[8], p[5], p[6], ROTS[rot]))
        want_c.append(True if R.DEEP + off < -1e-9 else None)  # (the last offset ends at touching)
        want_d.append(off < 0)
    out = host_check(cases)
    for i, (c, d) in enumerate(zip(want_c, want_d)):
        assert c is None or (out[i, 0] > 0) == c, (i, cases[i][0], out[i])
        if d is not None:
            assert (out[i, 1] > 0) == d, (i, out[i])
    assert ((out[:, 2] == -1).all()) == (rot == "identity" and fam[0] in ("parallel_side", "stacked_caps", "rim_rim_diagonal"))


# ------------------------------------------------------------------ 4. hand cases
I3 = np.eye(3)
POST = (0.05, 0.1)
HAND = [("1cm_deep", 0.09, 0.0, 1, 1), ("half_mm", 0.0995, 0.0, 1, 0), ("2cm_apart", 0.12, 0.0, 0, 0),
        ("2cm_margin_3cm", 0.12, 0.03, 1, 0), ("touching_strict", 0.1, 0.0, 0, 0), ("touching_margin", 0.1, 1e-3, 1, 0)]


@pytest.mark.parametrize("case", HAND, ids=[h[0] for h in HAND])
def test_hand_cases(host_check, case):
    """two vertical posts (R 5 cm) side by side at centre distance x"""
    name, x, mg, nc, nd = case
    out = host_check([case_of(mg, np.array([x, 0.0, 0.03]), I3, *POST, I3, *POST)])
    assert (out[0, 0], out[0, 1]) == (nc, nd)
    assert 0.05 + 0.05 == 0.1  # touching is exact in binary
    if "touching" not in name:  # in general position too (touching is no longer exact there)
        out = host_check([case_of(mg, np.array([x, 0.0, 0.03]), I3, *POST, I3, *POST, Q)])
        assert (out[0, 0], out[0, 1]) == (nc, nd) and out[0, 2] != -1
    c, d = R.decide(R.vertical_sd(np.array([x, 0.0, 0.03]), *POST, *POST), mg)
    assert (int(c), int(d)) == (nc, nd)


# ------------------------------------------------------------------ 5. scene creation
def test_pair_supported_is_symmetric_and_capsule_cylinder_is_not(tmp_path):
    src = tmp_path / "ps.cpp"
    src.write_text('#include <cstdio>\n#include "sspp_device.h"\nint main() { std::printf("%d %d %d %d\\n", '
                   '(int)sspd::pair_supported(5, 5), (int)sspd::pair_supported(3, 5), (int)sspd::pair_supported(5, 3), '
                   '(int)sspd::pair_supported(5, 6)); }\n')
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    exe = str(tmp_path / "ps")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "sspp_amd", "csrc"), str(src), "-o", exe])
    assert subprocess.check_output([exe], text=True).split() == ["1", "0", "0", "1"]


def test_cylinder_cylinder_scene_is_accepted_by_the_pair_check(tmp_path):
    """A mover cylinder beside a post passed the loader and was refused by the pair check with
    (-5) before; now the pair check passes (scene creation then goes on to the device)."""
    import sspp_amd as S
    from tests import cylcyl_scenes as CC
    from tests import synth_scenes as Y
    st, bodies = CC.sspp_cyl_mover()
    path = str(tmp_path / "cc.xml")
    with open(path, "w") as f:
        f.write(Y.mjcf(st, bodies))
    m = S.Model(path)
    import torch
    if torch.cuda.is_available():
        assert S.Scene(m, 0, 7).info()["n_pairs"] == 4
    else:  # without a device only the upload of the finished tables may fail: its first hipMalloc,
        # and a failed allocation is SSPP_E_NOMEM (-4) whatever HIP's reason
        with pytest.raises(S.SsppError, match=r"\(-4\).*no ROCm-capable device"):
            S.Scene(m, 0, 7)


def test_kernel_selection_takes_the_closed_forms_for_vertical_pairs(tmp_path):
    """sspk::kscene and tsp_cbm on hand-built scene records (tests/cylcyl/check_dispatch.cpp, host
    only): CB = 3 exactly when a cylinder-cylinder pair is present and every cylinder pair is
    vertical / upright, 2 for upright cylinder-box pairs alone, 1 as soon as one geom is tilted or
    the generic kernels are forced."""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    exe = str(tmp_path / "check_dispatch")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "sspp_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "cylcyl", "check_dispatch.cpp"), "-o", exe])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    # per row: (cylbox bits, cbup, upright, cbm) by default, then with the generic kernels forced
    want = [(5, 3), (4, 3), (5, 1), (4, 1), (1, 2), (5, 1)]
    assert len(rows) == len(want)
    for r, (bits, cbm) in zip(rows, want):
        assert (r[0], r[3]) == (bits, cbm), r
        assert r[1] == (cbm != 1) and (r[4], r[5], r[7]) == (bits, 0, 1), r
