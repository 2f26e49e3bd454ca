"""Reference of the contact report — TEST INFRASTRUCTURE ONLY.

Per pair and pose: `contact` (what sspd::collide<false> counts) and `deep` (contacts below -1e-3).
  * pairs of oracle-known types: the CPU oracle on a copy of the model with every geom but the
    pair's two made non-collidable — O.Scene(...).contacts(q) -> (n, cost, nd): contact = n, deep = nd;
  * pairs with a capsule: tests/capsule_ref.collide on the oracle's world poses;
  * cylinder-cylinder pairs: tests/cylcyl_scenes.pair_sd (the brute-force signed distance).
The two brute-force references have near bands (1e-9, cylcyl_ref.BAND): a pose inside one is
reported in `near` and left out by the caller (at most MAX_NEAR poses).
"""
import numpy as np

from oracle import oracle as O
from tests import capsule_ref as CR
from tests import capsule_scenes as CS
from tests import cylcyl_ref as CCR
from tests import cylcyl_scenes as CC
from tests import synth_scenes as Y

N_POSES = 257
MAX_NEAR = 2
CAP_BAND = 1e-9
CAPSULE, CYL = CS.CAPSULE, Y.CYLINDER


def qpos_poses(seed=1, n=N_POSES):
    """The QPOS recipe: x ~ U(-0.1, 1.1), y ~ U(-0.25, 0.25), z ~ U(0, 0.4), a random unit quaternion."""
    rng = np.random.default_rng(seed)
    q = np.empty((n, 7))
    q[:, 0] = rng.uniform(-0.1, 1.1, n)
    q[:, 1] = rng.uniform(-0.25, 0.25, n)
    q[:, 2] = rng.uniform(0.0, 0.4, n)
    w = rng.normal(size=(n, 4))
    q[:, 3:] = w / np.linalg.norm(w, axis=1, keepdims=True)
    return q


def qpos_poses_d(dof, qpos0, seed=1, n=N_POSES):
    """The recipe for a window of `dof` values: body 0 as above; a second body's driven entries
    (dof 9: x, y) jittered about qpos0 by U(-0.15, 0.15)."""
    q = qpos_poses(seed, n)
    if dof <= 7:
        return np.ascontiguousarray(q[:, :dof])
    rng = np.random.default_rng(seed + 1000)
    extra = np.asarray(qpos0, float)[7:dof] + rng.uniform(-0.15, 0.15, (n, dof - 7))
    return np.ascontiguousarray(np.concatenate([q, extra], 1))


def body_poses(seed=1, n=N_POSES):
    """The BODY recipe: x ~ U(-0.35, 0.3), y ~ U(-0.3, 0.3), z ~ U(0, 0.4), yaw ~ U(-1.6, 1.6)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.35, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(0.0, 0.4, n),
                     rng.uniform(-1.6, 1.6, n)], 1)


def moving_bodies(ref, mode, arg):
    if mode == 0:
        return [b for b in range(len(ref["body_parent"])) if ref["body_jnt_type"][b] == 0 and ref["body_qpos_adr"][b] < arg]
    return [int(arg)]


def _collidable(ref):
    """every collidable pair (g1 < g2) of a scene whose bodies all hang off the world"""
    gb, ct, ca = ref["geom_body"], ref["geom_contype"], ref["geom_conaffinity"]
    for g1 in range(len(gb)):
        for g2 in range(g1 + 1, len(gb)):
            if gb[g1] != gb[g2] and ((ct[g1] & ca[g2]) or (ct[g2] & ca[g1])):
                yield g1, g2


def columns(ref, mode, arg):
    """The report's columns [(g1, g2)], g1 < g2, in scene_build's order: (g1, g2) order, and in QPOS
    mode grouped (stably) by the pair's moving geom — g1 when it moves, else g2."""
    mv = set(moving_bodies(ref, mode, arg))
    gb = ref["geom_body"]
    pairs = [(a, b) for a, b in _collidable(ref) if gb[a] in mv or gb[b] in mv]
    if mode == 0:
        pairs.sort(key=lambda p: p[0] if gb[p[0]] in mv else p[1])
    return pairs


def static_columns(ref, mode, arg):
    mv = set(moving_bodies(ref, mode, arg))
    gb = ref["geom_body"]
    return [(a, b) for a, b in _collidable(ref) if gb[a] not in mv and gb[b] not in mv]


def pair_type(ref, a, b):
    return tuple(sorted((int(ref["geom_type"][a]), int(ref["geom_type"][b]))))


def _brute(ref, fk_scene, a, b, qs):
    """(contact [N], deep [N], near [N]) of a capsule or cylinder-cylinder pair from world poses"""
    gt = ref["geom_type"]
    mg = max(ref["geom_margin"][a], ref["geom_margin"][b])
    xp, xm = CS.fk_all(fk_scene, qs)
    if CAPSULE in (gt[a], gt[b]):
        g1, g2 = (a, b) if gt[a] <= gt[b] else (b, a)
        nc, nd, d, _ = CS.pair_results(ref, [(g1, g2, mg)], xp, xm)[0]
        return nc.astype(np.uint8), nd.astype(np.uint8), CR.decisive_gap(d, mg) < CAP_BAND
    (d, _), = CC.pair_sd(ref, [(a, b, mg)], xp, xm)
    (dd, _), = CC.pair_sd(ref, [(a, b, mg)], xp, xm, deep=True)
    # collide<true>: deep iff in contact (dist < margin) and dist < -1e-3; the margins here are >= 0
    c = d < mg
    near = (np.abs(d - mg) < CCR.BAND) | (np.abs(dd - CCR.DEEP) < CCR.BAND)
    return c.astype(np.uint8), (c & (dd < CCR.DEEP)).astype(np.uint8), near


def oracle_model(ref):
    """the model the oracle can hold: capsules off, and the bits cylinder-cylinder pairs meet on"""
    m = dict(ref)
    gt = np.asarray(ref["geom_type"])
    cc = any(gt[a] == CYL and gt[b] == CYL for a, b in _collidable(ref))
    ct, ca = np.asarray(ref["geom_contype"]), np.asarray(ref["geom_conaffinity"])
    if cc:
        ct, ca = ct & ~CC.CC_BITS, ca & ~CC.CC_BITS
    m["geom_contype"] = np.where(gt == CAPSULE, 0, ct)
    m["geom_conaffinity"] = np.where(gt == CAPSULE, 0, ca)
    return m


def pair_counts(ref, mode, arg, pairs, qs, count_static=False):
    """contact [N, P], deep [N, P] (uint8) and near [N] (bool) of the pairs [(g1, g2)] at poses qs."""
    qs = np.asarray(qs, float)
    N, P = len(qs), len(pairs)
    contact, deep = np.zeros((N, P), np.uint8), np.zeros((N, P), np.uint8)
    near = np.zeros(N, bool)
    ng = len(ref["geom_type"])
    fk_scene = None
    for k, (a, b) in enumerate(pairs):
        t = pair_type(ref, a, b)
        if CAPSULE in t or t == (CYL, CYL):
            if fk_scene is None:
                fk_scene = O.Scene(oracle_model(ref), mode, arg)
            contact[:, k], deep[:, k], nr = _brute(ref, fk_scene, a, b, qs)
            near |= nr
            continue
        sc = O.Scene(Y.with_geoms_off(ref, [g for g in range(ng) if g not in (a, b)]), mode, arg)
        for i, q in enumerate(qs):
            n, _, nd = sc.contacts(q, count_static=count_static)
            contact[i, k], deep[i, k] = n, nd
    return contact, deep, near


def static_counts(ref, mode, arg):
    """[(g1, g2, contact, deep)] of the env-env pairs at the model's own poses"""
    q0 = np.asarray(ref["qpos0"], float)[:arg] if mode == 0 else np.zeros(4)
    pairs = static_columns(ref, mode, arg)
    c, d, near = pair_counts(ref, mode, arg, pairs, q0[None], count_static=True)
    assert not near.any()
    return [(a, b, int(c[0, k]), int(d[0, k])) for k, (a, b) in enumerate(pairs)]


def assert_not_vacuous(ref, pairs, contact, deep, min_each=4, want_multi=True, want_deep_gt=True, want_shallow=True):
    """From the reference alone: every pair type has >= min_each touching and free poses; a
    touching-not-deep entry, an entry with deep > contact and a pose with two pairs touching exist."""
    types = {}
    for k, (a, b) in enumerate(pairs):
        t = pair_type(ref, a, b)
        tch = types.setdefault(t, [np.zeros(len(contact), bool), np.zeros(len(contact), bool)])
        tch[0] |= contact[:, k] > 0
        tch[1] |= contact[:, k] == 0
    for t, (tc, fr) in types.items():
        assert tc.sum() >= min_each and fr.sum() >= min_each, (t, int(tc.sum()), int(fr.sum()))
    if want_shallow:
        assert ((contact > 0) & (deep == 0)).any()
    if want_deep_gt:
        assert (deep > contact).any()
    if want_multi:
        assert ((contact > 0).sum(1) >= 2).any()
    return sorted(types)
