"""Capsule colliders on the CPU: the numpy reference (tests/capsule_ref.py) against an independent
distance per pair type and hand-computed cases, the host build of the device code
(sspd::collide, sspp_amd/csrc/sspp_device.h) against the reference, and the loader (capsules,
`fromto`).  MuJoCo is not available: the rules are the restated ones of DESIGN.md §4.

Random cases: 20 000 pairs per type placed 1e-8 .. 1e-1 m on either side of a decision threshold
(the margin, or the deep threshold -1e-3), margins 0 / 1 mm / 10 mm.  A case whose distance lies
within 1e-9 of a threshold is left out of the comparisons (rounding may flip it); the generator
places at most 0.1 % there, which each test asserts from the reference alone.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import mjcf_ref
from tests import capsule_ref as R
from tests import capsule_scenes as CS
from tests import synth_scenes as Y

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
N = 20000
EXCL, CAP_LEFT_OUT = 1e-9, 0.001
MARGINS = np.array([0.0, 1e-3, 1e-2])


# ------------------------------------------------------------------ case generation
def rand_quat(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def mats(q):
    return np.array([CS.quat2mat(x) for x in q])


def targets(rng, n):
    """(margin, target signed distance): a threshold +- a gap of 1e-8 .. 1e-1."""
    margin = MARGINS[rng.integers(0, 3, n)]
    thr = np.where(rng.random(n) < 0.5, margin, R.DEEP)
    gap = 10.0 ** rng.uniform(-8, -1, n) * rng.choice([-1.0, 1.0], n)
    return margin, thr + gap


def perp_unit(rng, a):
    v = np.cross(a, rng.normal(size=a.shape))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


M = 2 * N


def first_n(c, ok):
    """The first N usable cases of the M drawn."""
    idx = np.flatnonzero(ok)[:N]
    assert len(idx) == N
    return {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def gen_plane_capsule(seed=11):
    rng = np.random.default_rng(seed)
    margin, tgt = targets(rng, N)
    pp, pm = rng.uniform(-0.2, 0.2, (N, 3)), mats(rand_quat(rng, N))
    n = R.zcol(pm)
    cm = mats(rand_quat(rng, N))
    # a quarter lying along the plane, exactly or within 1e-6 rad: both ends near the threshold
    lying = rng.random(N) < 0.25
    t = perp_unit(rng, n)
    tilt = np.where(rng.random(N) < 0.5, 0.0, 10.0 ** rng.uniform(-9, -6, N))[:, None]
    a = t + tilt * n
    cm[lying] = mats(np.array([CS.quat_z_to(x) for x in a[lying]]))
    h = rng.uniform(0.03, 0.3, N)
    low = h * np.abs(R.dot(n, R.zcol(cm)))                 # the lower end's depth below the centre
    height = low + rng.uniform(0.12, 0.3, N)             # (above every target distance: r > 0)
    cp = pp + height[:, None] * n + 0.3 * rng.normal(size=(N, 1)) * perp_unit(rng, n)
    r = (R.dot(n, cp - pp) - low) - tgt
    cs = np.stack([r, h, np.zeros(N)], 1)
    assert (r > 0).all()
    return dict(t1=R.PLANE, t2=R.CAPSULE, p1=pp, m1=pm, s1=np.tile([0.0, 0.0, 1.0], (N, 1)), p2=cp, m2=cm, s2=cs,
                margin=margin)


def gen_sphere_capsule(seed=12):
    rng = np.random.default_rng(seed)
    margin, tgt = targets(rng, N)
    cp, cm = rng.uniform(-0.2, 0.2, (N, 3)), mats(rand_quat(rng, N))
    a, h = R.zcol(cm), rng.uniform(0.03, 0.3, N)
    along = rng.uniform(-1.6, 1.6, N) * h                   # beside the segment and beyond its ends
    sp = cp + along[:, None] * a + rng.uniform(0.14, 0.3, N)[:, None] * perp_unit(rng, a)
    D = R.point_seg_independent(sp, cp, a, h)
    rs = rng.uniform(0.01, 0.02, N)
    r = D - tgt - rs
    assert (r > 0).all()
    return dict(t1=R.SPHERE, t2=R.CAPSULE, p1=sp, m1=mats(rand_quat(rng, N)), s1=np.stack([rs, rs * 0, rs * 0], 1),
                p2=cp, m2=cm, s2=np.stack([r, h, np.zeros(N)], 1), margin=margin)


def gen_capsule_capsule(seed=13):
    """60 % general, 15 % exactly parallel (the same rotation), 5 % exactly antiparallel, 10 %
    within 1e-12 .. 1e-9 rad of parallel (the parallel branch: its end tests are exact to
    angle x length < 1e-9 m), 10 % at 1e-7 .. 1e-2 rad (the general branch at its worst
    conditioning).  Between lies the switch-over (|det| = 1e-15, 3e-8 rad), where the end tests
    of a 0.3 m segment are off by up to 1e-8 m: a property of the rule, not sampled here."""
    rng = np.random.default_rng(seed)
    N = M                                                   # (drawn; the first 20 000 usable are kept)
    margin, tgt = targets(rng, N)
    q1 = rand_quat(rng, N)
    m1 = mats(q1)
    a1 = R.zcol(m1)
    kind = rng.choice(5, N, p=[0.6, 0.15, 0.05, 0.1, 0.1])
    m2 = mats(rand_quat(rng, N))
    m2[kind == 1] = m1[kind == 1]
    anti = m1[kind == 2].reshape(-1, 3, 3).copy()
    anti[:, :, 1:] *= -1.0                                  # y and z columns negated: a proper rotation
    m2[kind == 2] = anti.reshape(-1, 9)
    ang = np.where(kind == 3, 10.0 ** rng.uniform(-12, -9, N), 10.0 ** rng.uniform(-7, -2, N))
    near = (kind == 3) | (kind == 4)
    d = a1 + ang[:, None] * perp_unit(rng, a1)
    m2[near] = mats(np.array([CS.quat_z_to(x) for x in d[near]]))
    a2 = R.zcol(m2)
    h1, h2 = rng.uniform(0.03, 0.3, N), rng.uniform(0.03, 0.3, N)
    p1 = rng.uniform(-0.2, 0.2, (N, 3))
    p2 = p1 + (rng.uniform(-1.3, 1.3, N) * (h1 + h2))[:, None] * a1 + rng.uniform(0.13, 0.35, N)[:, None] * perp_unit(rng, a1)
    D = R.seg_seg_independent(p1, a1, h1, p2, a2, h2)
    ok = D > 0.12                                           # (above every target distance: radii > 0)
    rsum = D - tgt
    f = rng.uniform(0.3, 0.7, N)
    c = dict(t1=R.CAPSULE, t2=R.CAPSULE, p1=p1, m1=m1, s1=np.stack([f * rsum, h1, h1 * 0], 1), p2=p2, m2=m2,
             s2=np.stack([(1 - f) * rsum, h2, h2 * 0], 1), margin=margin, kind=kind)
    return first_n(c, ok)


def gen_capsule_box(seed=14):
    """35 % general, 20 % along a box axis exactly (parallel to a face and an edge), 15 % within
    1e-9 .. 1e-4 rad of a box axis, 15 % piercing the box, 15 % general but placed beside a face,
    edge or corner in the box's own coordinates."""
    rng = np.random.default_rng(seed)
    N = M
    margin, tgt = targets(rng, N)
    bp, bq = rng.uniform(-0.2, 0.2, (N, 3)), rand_quat(rng, N)
    bm = mats(bq)
    Bx = bm.reshape(N, 3, 3)
    e = rng.uniform(0.03, 0.15, (N, 3))
    kind = rng.choice(5, N, p=[0.35, 0.2, 0.15, 0.15, 0.15])
    cm = mats(rand_quat(rng, N))
    k = rng.integers(0, 3, N)
    axis = Bx[np.arange(N), :, k]                            # the box's axis k (a column), world frame
    other = Bx[np.arange(N), :, (k + 1) % 3]
    al = (kind == 1) | (kind == 2)
    tilt = np.where(kind == 2, 10.0 ** rng.uniform(-9, -4, N), 0.0)[:, None]
    cm[al] = mats(np.array([CS.quat_z_to(x) for x in (axis + tilt * other)[al]]))
    exact = kind == 1                                        # the frame built from the box's own columns
    cyc = np.stack([Bx[np.arange(N), :, (k + 1) % 3], Bx[np.arange(N), :, (k + 2) % 3], axis], 2)
    cm[exact] = cyc.reshape(N, 9)[exact]
    h = rng.uniform(0.03, 0.3, N)
    local = rng.uniform(-1.5, 1.5, (N, 3)) * e             # beside a face, an edge or a corner ...
    j = rng.integers(0, 3, N)
    local[np.arange(N), j] = rng.choice([-1.0, 1.0], N) * (e[np.arange(N), j] + rng.uniform(0.12, 0.3, N))  # ... outside
    local[kind == 3] = (rng.uniform(-0.8, 0.8, (N, 3)) * e)[kind == 3]
    far = rng.normal(size=(N, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * (np.linalg.norm(e, axis=1) + h + rng.uniform(0.03, 0.2, N))[:, None]
    local = np.where((kind == 0)[:, None], far, local)
    cp = bp + np.einsum("nij,nj->ni", Bx, local)
    P, d = R.to_frame(bm, cp - bp), R.to_frame(bm, R.zcol(cm))
    D = R.seg_box_independent(P, d, e, h)
    pierce = kind == 3
    r = np.where(pierce, rng.uniform(0.005, 0.05, N), D - tgt)
    ok = pierce | (D > 0.12)
    c = dict(t1=R.CAPSULE, t2=R.BOX, p1=cp, m1=cm, s1=np.stack([r, h, h * 0], 1), p2=bp, m2=bm, s2=e, margin=margin,
             kind=kind, D=D)
    return first_n(c, ok)


GENERATORS = {"plane_capsule": gen_plane_capsule, "sphere_capsule": gen_sphere_capsule,
              "capsule_capsule": gen_capsule_capsule, "capsule_box": gen_capsule_box}


@pytest.fixture(scope="module")
def cases():
    """Every type's seeded cases with the reference's results, computed once."""
    out = {}
    for name, gen in GENERATORS.items():
        c = gen()
        c["ref"] = R.collide(c["t1"], c["p1"], c["m1"], c["s1"], c["t2"], c["p2"], c["m2"], c["s2"], c["margin"])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[name] = c
    return out


def kept(c):
    """The cases compared: every test the reference ran is >= 1e-9 from both thresholds; at most
    0.1 % may be left out, by the reference alone."""
    keep = R.decisive_gap(c["ref"][2], c["margin"]) >= EXCL
    assert (~keep).mean() <= CAP_LEFT_OUT, (~keep).mean()
    return keep


# ------------------------------------------------------------------ reference vs independent
def independent_min_dist(name, c):
    a2 = R.zcol(c["m2"])
    if name == "plane_capsule":
        n = R.zcol(c["m1"])
        return R.dot(n, c["p2"] - c["p1"]) - c["s2"][:, 1] * np.abs(R.dot(n, a2)) - c["s2"][:, 0]
    if name == "sphere_capsule":
        return R.point_seg_independent(c["p1"], c["p2"], a2, c["s2"][:, 1]) - c["s1"][:, 0] - c["s2"][:, 0]
    if name == "capsule_capsule":
        return (R.seg_seg_independent(c["p1"], R.zcol(c["m1"]), c["s1"][:, 1], c["p2"], a2, c["s2"][:, 1]) -
                c["s1"][:, 0] - c["s2"][:, 0])
    P, d = R.to_frame(c["m2"], c["p1"] - c["p2"]), R.to_frame(c["m2"], R.zcol(c["m1"]))
    return R.seg_box_independent(P, d, c["s2"], c["s1"][:, 1]) - c["s1"][:, 0]


@pytest.mark.parametrize("name", list(GENERATORS))
def test_reference_agrees_with_independent_distance(cases, name):
    c = cases[name]
    n = len(c["margin"])
    assert n == N
    nc, nd, d = c["ref"]
    di = independent_min_dist(name, c)
    keep = kept(c) & (np.minimum(np.abs(di - c["margin"]), np.abs(di - R.DEEP)) >= EXCL)
    assert (~keep).mean() <= CAP_LEFT_OUT
    contact = di <= c["margin"]
    deep = contact & (di < R.DEEP)
    assert np.array_equal((nc > 0)[keep], contact[keep])
    # the parallel branch stops after two contacts: ends 1 and 2 touching but not deep can hide a
    # deep contact of ends 3 and 4 (a short capsule inside a long one's span); that is the rule
    hidden = np.zeros(n, bool)
    if name == "capsule_capsule":
        hidden = np.isnan(d[:, 2]) & ~np.isnan(d[:, 1]) & (nd == 0) & deep
        assert hidden.sum() < 0.01 * n
    assert np.array_equal((nd > 0)[keep & ~hidden], deep[keep & ~hidden])
    assert not (nd > 0)[keep & ~deep].any()
    # both outcomes of both decisions, and the generator's special families, are all there
    assert 0.2 < contact.mean() < 0.8 and 0.1 < deep.mean() < 0.8
    if name == "plane_capsule":
        assert (nc == 2).sum() > 1000 and (nc == 1).sum() > 1000
        upper = di + 2 * c["s2"][:, 1] * np.abs(R.dot(R.zcol(c["m1"]), R.zcol(c["m2"])))
        k2 = keep & (np.abs(upper - c["margin"]) >= EXCL)
        assert np.array_equal((nc == 2)[k2], (upper <= c["margin"])[k2])
    if name == "capsule_capsule":
        par = ~np.isnan(d[:, 1])
        assert par.sum() > 0.25 * n and (nc == 2).sum() > 1000
        assert set(np.unique(c["kind"])) == {0, 1, 2, 3, 4}
        assert par[np.isin(c["kind"], (1, 2, 3))].all() and not par[np.isin(c["kind"], (0, 4))].any()
        # the numbers agree too, not only the decisions
        one = ~par
        assert np.abs(d[one, 0] - di[one]).max() < 1e-12
    if name == "capsule_box":
        assert set(np.unique(c["kind"])) == {0, 1, 2, 3, 4}
        assert (c["D"][c["kind"] == 3] == 0.0).all() and (nd[c["kind"] == 3] == 1).all()
        assert np.abs(d[:, 0] - di).max() < 1e-9


# ------------------------------------------------------------------ hand cases
IDENT = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
Z_TO_X = CS.quat2mat(CS.quat_z_to((1, 0, 0)))
Z_TO_Y = CS.quat2mat(CS.quat_z_to((0, 1, 0)))
HAND = [
    # plane z = 0; capsule r = 0.05, h = 0.1
    ("standing 1 cm in", R.PLANE, (0, 0, 0), IDENT, (0, 0, 1), R.CAPSULE, (0, 0, 0.14), IDENT, (0.05, 0.1, 0), 0.0, 1, 1),
    ("lying 0.5 mm in", R.PLANE, (0, 0, 0), IDENT, (0, 0, 1), R.CAPSULE, (0.3, 0, 0.0495), Z_TO_X, (0.05, 0.1, 0), 0.0, 2, 0),
    ("lying 1 cm in", R.PLANE, (0, 0, 0), IDENT, (0, 0, 1), R.CAPSULE, (0.3, 0, 0.04), Z_TO_X, (0.05, 0.1, 0), 0.0, 2, 2),
    # two capsules r = 0.05, h = 0.1, axes 0.08 apart: 2 cm in
    ("crossed", R.CAPSULE, (0, 0, 0), Z_TO_X, (0.05, 0.1, 0), R.CAPSULE, (0, 0, 0.08), Z_TO_Y, (0.05, 0.1, 0), 0.0, 1, 1),
    ("side by side", R.CAPSULE, (0, 0, 0), Z_TO_X, (0.05, 0.1, 0), R.CAPSULE, (0, 0.08, 0), Z_TO_X, (0.05, 0.1, 0), 0.0, 2, 2),
    # sphere r = 0.03 beyond the end of a z capsule (r = 0.05, h = 0.1): 0.2 - 0.1 - 0.08 = 0.02 clear
    ("sphere clear", R.SPHERE, (0, 0, 0.2), IDENT, (0.03, 0, 0), R.CAPSULE, (0, 0, 0), IDENT, (0.05, 0.1, 0), 0.0, 0, 0),
    ("sphere in margin", R.SPHERE, (0, 0, 0.2), IDENT, (0.03, 0, 0), R.CAPSULE, (0, 0, 0), IDENT, (0.05, 0.1, 0), 0.03, 1, 0),
    # cube e = 0.1; capsule pointing away from the edge x = y = 0.1 along (1, 1, 0) / sqrt 2, its
    # near end 0.05 from the edge: d_seg = 0.05
    ("edge r 0.051", R.CAPSULE, tuple(np.array([0.1, 0.1, 0.02]) + 0.15 * np.array([1, 1, 0]) / np.sqrt(2)),
     CS.quat2mat(CS.quat_z_to((1, 1, 0))), (0.051, 0.1, 0), R.BOX, (0, 0, 0), IDENT, (0.1, 0.1, 0.1), 0.0, 1, None),
    ("edge r 0.049", R.CAPSULE, tuple(np.array([0.1, 0.1, 0.02]) + 0.15 * np.array([1, 1, 0]) / np.sqrt(2)),
     CS.quat2mat(CS.quat_z_to((1, 1, 0))), (0.049, 0.1, 0), R.BOX, (0, 0, 0), IDENT, (0.1, 0.1, 0.1), 0.0, 0, 0),
    ("through the box", R.CAPSULE, (0.03, -0.02, 0.01), IDENT, (0.02, 0.3, 0), R.BOX, (0, 0, 0), IDENT, (0.1, 0.1, 0.1), 0.0, 1, 1),
]


def hand_arrays():
    c = dict(p1=[], m1=[], s1=[], p2=[], m2=[], s2=[], margin=[], t1=[], t2=[])
    for _, t1, p1, m1, s1, t2, p2, m2, s2, mg, _, _ in HAND:
        for k, v in zip(("t1", "p1", "m1", "s1", "t2", "p2", "m2", "s2", "margin"), (t1, p1, m1, s1, t2, p2, m2, s2, mg)):
            c[k].append(v)
    return c


@pytest.mark.parametrize("case", HAND, ids=[h[0] for h in HAND])
def test_hand_cases(case):
    _, t1, p1, m1, s1, t2, p2, m2, s2, mg, want_nc, want_nd = case
    nc, nd, d = R.collide(t1, p1, m1, s1, t2, p2, m2, s2, mg)
    assert nc[0] == want_nc
    if want_nd is not None:
        assert nd[0] == want_nd
    # away from every rounding boundary (r = 0.051 at d_seg = 0.05 sits on the deep threshold, so
    # that case pins the contact alone)
    assert (R.decisive_gap(d, mg)[0] if want_nd is not None else np.nanmin(np.abs(d - mg))) > 1e-6


def test_hand_distances():
    """The hand cases' distances themselves."""
    d = lambda i: R.collide(*HAND[i][1:10])[2][0]
    np.testing.assert_allclose(d(0), [0.19, -0.01], atol=1e-15)
    np.testing.assert_allclose(d(1), [-0.0005, -0.0005], atol=1e-15)
    np.testing.assert_allclose(d(3)[0], -0.02, atol=1e-15)
    np.testing.assert_allclose(d(4)[:2], [-0.02, -0.02], atol=1e-15)
    assert np.isnan(d(4)[2:]).all()
    np.testing.assert_allclose(d(5)[0], 0.02, atol=1e-15)
    np.testing.assert_allclose(d(7)[0], 0.05 - 0.051, atol=1e-15)
    np.testing.assert_allclose(d(9)[0], -0.02, atol=1e-15)


# ------------------------------------------------------------------ host build of the device code
def hexrow(*parts):
    return " ".join(float(x).hex() for p in parts for x in np.ravel(p))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("capsule_host")
    exe = str(d / "check_capsule")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "the host build of the device code needs hipcc"
    subprocess.check_call([hipcc, "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "sspp_amd", "csrc"),
                           os.path.join(HERE, "capsule", "check_capsule.cpp"), "-o", exe])

    def run(c):
        path = str(d / "cases.txt")
        n = len(c["margin"])
        with open(path, "w") as f:
            for i in range(n):
                t1 = c["t1"][i] if np.ndim(c["t1"]) else c["t1"]
                t2 = c["t2"][i] if np.ndim(c["t2"]) else c["t2"]
                f.write(hexrow([t1, t2, c["margin"][i]], c["p1"][i], c["m1"][i], c["s1"][i], c["p2"][i], c["m2"][i],
                               c["s2"][i]) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out = np.array([[float(x) for x in line.split()] for line in r.stdout.splitlines()])
        assert out.shape == (n, 6)
        return out[:, 0].astype(int), out[:, 1].astype(int), out[:, 2:]

    return run


@pytest.mark.parametrize("name", list(GENERATORS))
def test_host_build_matches_reference(cases, host_check, name):
    """sspd::collide<false> / collide<true> on the seeded cases: counts equal, every distance within
    1e-12 of the reference's, the same tests run."""
    c = cases[name]
    nc, nd, d = c["ref"]
    hc, hd, hdist = host_check(c)
    keep = kept(c)
    ran = ~np.isnan(d)
    assert np.array_equal(np.isnan(hdist[keep, :d.shape[1]]), ~ran[keep])
    assert np.isnan(hdist[:, d.shape[1]:]).all()
    assert np.abs(hdist[:, :d.shape[1]][ran] - d[ran]).max() <= 1e-12
    assert np.array_equal(hc[keep], nc[keep]) and np.array_equal(hd[keep], nd[keep])


def test_host_build_hand_cases(host_check):
    c = hand_arrays()
    c = {k: np.array(v, float) if k not in ("t1", "t2") else v for k, v in c.items()}
    hc, hd, _ = host_check(c)
    for i, h in enumerate(HAND):
        assert hc[i] == h[10], h[0]
        if h[11] is not None:
            assert hd[i] == h[11], h[0]


# ------------------------------------------------------------------ the composed TSP reference
@pytest.mark.parametrize("cp", [40, 65])
def test_composed_tsp_reference_reproduces_the_oracle(tmp_path, cp):
    """tests/capsule_scenes.py's composition (waypoint grid, canonical sums, floor term, status,
    cost) on a capsule-free scene is the oracle's tsp_score to 1e-12: that pins the grid the GPU
    capsule tests compare on."""
    from oracle import oracle as O
    path = write(tmp_path, "boxes.xml", CS.tsp_no_capsule())
    ref = mjcf_ref.load(path)
    osc = O.Scene(ref, 1, ref["body_names"].index("mover"))
    mean = np.array([Y.TSP_START + (Y.TSP_END - Y.TSP_START) * (i + 1) / 3 for i in range(2)])
    vias = O.sample_tsp(mean, np.full((2, 4), 0.15), Y.TSP_LO, Y.TSP_HI, 0.0, 7, 5, 256)
    want = O.tsp_score(osc, Y.TSP_START, Y.TSP_END, vias, cp)
    got = CS.tsp_compose(osc, ref, [], Y.TSP_START, Y.TSP_END, vias, cp)
    assert 16 <= int(want[3].sum()) <= 240
    for a, b in zip(want, got[:5]):
        assert np.abs(np.asarray(a, float) - np.asarray(b, float)).max() <= 1e-12


# ------------------------------------------------------------------ loader
def write(tmp_path, name, xml):
    p = tmp_path / name
    p.write_text(xml)
    return str(p)


def segment_ends(arrays, g):
    """World ends of geom g's segment (the scenes' geoms hang off the world or a body at the
    identity): pos +- size[1] * (z axis of quat)."""
    a = CS.quat2mat(arrays["geom_quat"][g])[[2, 5, 8]]
    p, h = np.asarray(arrays["geom_pos"][g]), arrays["geom_size"][g][1]
    return p + h * a, p - h * a


def test_size_capsules_load_like_the_independent_reader(tmp_path):
    import sspp_amd as S
    st, bodies = CS.sspp_capsule_mover()
    path = write(tmp_path, "caps.xml", CS.mjcf(st, bodies))
    a = S.Model(path).arrays()
    Y.assert_loaders_agree(a, mjcf_ref.load(path))
    assert list(a["geom_type"]) == [0, 2, 3, 6, 3]


FROMTO = [((0.2, -0.2, 0.12), (0.3, -0.08, 0.32)),      # general
          ((0.42, 0.12, 0.36), (0.42, -0.02, 0.2)),     # pointing down
          ((0.1, 0.2, 0.1), (0.1, 0.2, 0.4)),           # +z: the identity
          ((0.1, 0.2, 0.4), (0.1, 0.2, 0.1)),           # -z exactly: the rotation by pi about x
          ((0.0, 0.0, 0.5), (1e-9, 0.0, 0.2))]          # within 4e-9 rad of -z


@pytest.mark.parametrize("gtype", [CS.CAPSULE, Y.CYLINDER])
def test_fromto_equals_explicit_pose(tmp_path, gtype):
    """fromto capsules and cylinders: the same world segment ends, to 1e-15, as the scene
    written with pos / quat / size, and those are the ends that were asked for."""
    import sspp_amd as S
    st = [CS.fromto(gtype, 0.03, a, b, name="g%d" % i, contype=2 ** i, conaffinity=2 ** i) for i, (a, b) in enumerate(FROMTO)]
    body = [Y.body("mover", (0, 0, 0.3), [Y.geom(Y.SPHERE, 0.01, name="m")])]
    got = S.Model(write(tmp_path, "ft.xml", CS.mjcf(st, body))).arrays()
    exp_path = write(tmp_path, "ex.xml", CS.mjcf(st, body, as_explicit=True))
    want = S.Model(exp_path).arrays()
    Y.assert_loaders_agree(want, mjcf_ref.load(exp_path))
    assert list(got["geom_type"][:5]) == [gtype] * 5
    for i, (a, b) in enumerate(FROMTO):
        assert got["geom_size"][i][0] == 0.03 and abs(got["geom_size"][i][1] - want["geom_size"][i][1]) <= 1e-15
        for e_got, e_want, e_asked in zip(segment_ends(got, i), segment_ends(want, i), (b, a)):
            assert np.abs(e_got - e_want).max() <= 1e-15
            assert np.abs(e_got - np.array(e_asked)).max() <= 1e-15
    np.testing.assert_array_equal(got["geom_quat"][2], [1, 0, 0, 0])
    np.testing.assert_array_equal(got["geom_quat"][3], [0, 1, 0, 0])


def test_loader_capsule_errors(tmp_path):
    import sspp_amd as S
    wrap = lambda g: '<mujoco><worldbody>%s<body name="b"><freejoint/><geom type="sphere" size="0.1"/></body></worldbody></mujoco>' % g
    bad = {"zero.xml": '<geom type="capsule" size="0.1" fromto="0 0 1 0 0 1"/>',
           "radius.xml": '<geom type="capsule" size="0 0.1"/>',
           "half.xml": '<geom type="capsule" size="0.1 0"/>',
           "nosize.xml": '<geom type="capsule" size="0.1"/>',
           "five.xml": '<geom type="capsule" size="0.1" fromto="0 0 1 0 0"/>'}
    for name, g in bad.items():
        with pytest.raises(S.SsppError, match=r"\(-3\)"):           # SSPP_E_SCENE
            S.Model(write(tmp_path, name, wrap(g)))
    for name, g in {"box.xml": '<geom type="box" size="0.1 0.1 0.1" fromto="0 0 0 0 0 1"/>',
                    "sphere.xml": '<geom type="sphere" size="0.1" fromto="0 0 0 0 0 1"/>',
                    "zaxis.xml": '<geom type="capsule" size="0.1 0.1" zaxis="0 1 0"/>',
                    "xyaxes.xml": '<geom type="capsule" size="0.1 0.1" xyaxes="1 0 0 0 1 0"/>'}.items():
        with pytest.raises(S.SsppError, match=r"\(-5\).*unsupported orientation attribute"):  # SSPP_E_UNSUPPORTED
            S.Model(write(tmp_path, name, wrap(g)))


def test_capsule_cylinder_pair_is_refused(tmp_path):
    import sspp_amd as S
    xml = CS.mjcf([Y.geom(Y.CYLINDER, (0.05, 0.1), (0.3, 0, 0.2), name="post")],
                  [Y.body("mover", (0, 0, 0.3), [CS.capsule(0.02, 0.05, name="m_cap")])])
    m = S.Model(write(tmp_path, "capcyl.xml", xml))
    with pytest.raises(S.SsppError, match=r"\(-5\).*'post'.*'m_cap'"):
        S.Scene(m, 0, 7)
