"""Worlds for arms on the host, without a GPU: tests/chain_world/check_world.cpp runs sspc::chain_build
with a world and the host half of sspp_chain_set_qpos / _set_body_pose (validate, edit a trial copy
of the chain's model data, chain_update, adopt), then the per-pose routines the chain kernels loop
over.  Checked: a re-posed chain's tables against chain_build on model data holding the new values
and against a chain loaded from a rewritten MJCF, byte for byte; the model's own world against
today's program (tests/chain/check_chain.cpp); kinematics and contact decisions against
tests/chain_world_ref.py (numpy, from the rule); static contacts; the refusals.  A second build of
the program runs under AddressSanitizer / UBSan (a stand-alone program).
"""
import numpy as np
import pytest

from tests import chain_host as H
from tests import chain_ref as R
from tests import chain_scenes as S
from tests import chain_world_host as WH
from tests import chain_world_ref as WR
from tests import chain_world_scenes as WS

FK_TOL = 1e-12  # the project's bar for tests/chain_ref.py (tests/test_chain_host.py)
FK_SEED, CONTACT_SEED = 501, 502


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chain_world") / "check_world")
    r = WH.build(out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("chain_world_files")


@pytest.fixture(scope="module")
def cells(tmp):
    out = {}
    for name, c in (("cell", WS.cell()), ("base", WS.base()), ("full", WS.full())):
        c["xml"] = H.write_xml(tmp, name, S.mjcf(c["world"]))
        c["m"] = R.flatten(c["world"])
        assert c["m"]["nq"] == c["nq"]
        out[name] = c
    out["cell"]["worlds"] = WS.cell_worlds(out["cell"]["m"]["qpos0"])
    out["base"]["worlds"] = WS.base_worlds(out["base"]["m"]["qpos0"])
    return out


def raw_ops(c, world):
    """the same world written into the model data as it is: normalised values, no update call"""
    names, m = c["m"]["body_names"], c["m"]
    ops = [] if world["qpos"] is None else [WH.op_qpos(WS.norm_world(world["qpos"], c["free"]), raw=True)]
    w = None if world["qpos"] is None else WS.norm_world(world["qpos"], c["free"])
    for name, pos, quat in world["poses"]:
        b = names.index(name)
        ops.append(WH.op_body(b, pos, WS.normq(quat), raw=True))
        if m["body_free"][b] >= 0:
            w = (m["qpos0"] if w is None else w).copy()
            w[m["body_free"][b]:m["body_free"][b] + 7] = list(pos) + WS.normq(quat)
            ops.append(WH.op_qpos(w, raw=True))
    return ops


def ref_of(c, world):
    m = WR.model(c["world"], world["poses"])
    return m, WR.world_qpos(m, world["qpos"], world["poses"])


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("cell,D,k", [("cell", 5, 1), ("cell", 5, 2), ("cell", 5, 3), ("base", 9, 1), ("base", 3, 1)])
def test_tables_equal_build_on_new_values(exe, tmp, cells, cell, D, k):
    c = cells[cell]
    world = c["worlds"][k]
    q = WS.cell_poses(D, 8, 3)
    own = WH.run(exe, c["xml"], D, [], q, tmp, tag="own")
    got = WH.run(exe, c["xml"], D, WH.world_ops(c["m"]["body_names"], world), q, tmp, tag="upd")
    want = WH.run(exe, c["xml"], D, raw_ops(c, world), q, tmp, tag="raw")
    assert got["rc"] == 0 and want["rc"] == 0 and all(o[0] == 0 for o in got["ops"]), (got["ops"], want["err"])
    assert got["epoch"] == len(got["ops"]) >= 1 and want["epoch"] == 0
    assert got["tables"] == want["tables"] and got["tables"] != own["tables"]
    for key in ("info", "pairs", "statics"):
        assert got[key] == want[key], key
    assert got["fk"].tobytes() == want["fk"].tobytes() and got["fk"].tobytes() != own["fk"].tobytes()
    # what no world changes: the pair table, every table's length, the driven set
    assert got["pairs"] == own["pairs"] and len(got["tables"]) == len(own["tables"])
    assert {k2: v for k2, v in got["info"].items() if k2 != "static_contacts"} == \
           {k2: v for k2, v in own["info"].items() if k2 != "static_contacts"}
    assert [s[:3] for s in got["statics"]] == [s[:3] for s in own["statics"]]
    np.testing.assert_array_equal(got["qpos"], WS.norm_world(world["qpos"], c["free"]))


def test_tables_equal_rewritten_mjcf(exe, tmp, cells):
    """where an MJCF expresses the world (a free body's pose, body poses): a fresh chain from the file"""
    c = cells["cell"]
    poses = [("block", WS.BLOCK_UP, [0.9, 0.1, -0.3, 0.2])] + c["worlds"][3]["poses"]
    q = WS.cell_poses(5, 8, 3)
    got = WH.run(exe, c["xml"], 5, WH.world_ops(c["m"]["body_names"], dict(qpos=None, poses=poses)), q, tmp, tag="upd2")
    xml2 = H.write_xml(tmp, "cell_rewritten", S.mjcf(WS.with_world(c["world"], {n: (p, qt) for n, p, qt in poses})))
    want = WH.run(exe, xml2, 5, [], q, tmp, tag="fresh")
    assert got["rc"] == 0 and want["rc"] == 0 and got["epoch"] == 5
    assert got["tables"] == want["tables"]
    assert got["fk"].tobytes() == want["fk"].tobytes() and got["hit"].tobytes() == want["hit"].tobytes()
    assert got["statics"] == want["statics"] and got["info"] == want["info"]
    np.testing.assert_array_equal(got["qpos"], want["qpos"])


def test_own_world_is_todays(exe, tmp, tmp_path_factory, cells):
    """a chain at the model's own world: the tables' outputs of the program without worlds, and a
    set_qpos(qpos0) changes no table byte"""
    old = str(tmp_path_factory.mktemp("chain_old") / "check_chain")
    r = H.build(old)
    assert r.returncode == 0, r.stderr[-4000:]
    for name in ("cell", "base", "full"):
        c = cells[name]
        q = WS.cell_poses(c["D"], 200, 9) if name != "base" else S.arm_poses(c["D"], 200, 9, 2.0, True)
        for cs in (0, 1):
            today = H.chain(old, c["xml"], c["D"], q, tmp, count_static=cs, tag="today")
            own = WH.run(exe, c["xml"], c["D"], [], q, tmp, count_static=cs, tag="own")
            same = WH.run(exe, c["xml"], c["D"], [WH.op_qpos(c["m"]["qpos0"])], q, tmp, count_static=cs, tag="same")
            assert today["rc"] == 0 and own["rc"] == 0 and same["rc"] == 0
            assert own["info"] == today["info"] and own["pairs"] == today["pairs"]
            assert own["fk"].tobytes() == today["fk"].tobytes() and own["hit"].tobytes() == today["hit"].tobytes()
            assert same["tables"] == own["tables"] and same["epoch"] == 1 and own["epoch"] == 0
            assert same["fk"].tobytes() == own["fk"].tobytes()


def test_entries_below_dof_and_full_dof(exe, tmp, cells):
    """world entries below dof are stored, returned and never read; with nq == dof a world changes nothing"""
    c = cells["cell"]
    q = WS.cell_poses(5, 4, 3)
    own = WH.run(exe, c["xml"], 5, [], q, tmp, tag="own")
    w = c["m"]["qpos0"].copy()
    w[:5] = [0.3, -0.2, 0.05, 1.0, -1.0]
    got = WH.run(exe, c["xml"], 5, [WH.op_qpos(w)], q, tmp, tag="below")
    assert got["tables"] == own["tables"] and got["epoch"] == 1
    np.testing.assert_array_equal(got["qpos"], w)
    f = cells["full"]
    q = WS.cell_poses(3, 4, 3)
    own = WH.run(exe, f["xml"], 3, [], q, tmp, tag="fown")
    got = WH.run(exe, f["xml"], 3, [WH.op_qpos([0.5, -0.4, 0.1])], q, tmp, tag="fall")
    assert got["ops"][0][0] == 0 and got["tables"] == own["tables"] and got["fk"].tobytes() == own["fk"].tobytes()
    np.testing.assert_array_equal(got["qpos"], [0.5, -0.4, 0.1])


# ------------------------------------------------------------------ kinematics and decisions
def test_fk_against_reference(exe, tmp, cells):
    c = cells["cell"]
    q = WS.cell_poses(5, 1000, FK_SEED)
    for k, world in enumerate(c["worlds"]):
        got = WH.run(exe, c["xml"], 5, WH.world_ops(c["m"]["body_names"], world), q, tmp, tag="fk%d" % k)
        m, w = ref_of(c, world)
        gpos, gmat = WR.fk(m, w, q, 5)
        err = max(np.abs(got["fk"][:, :, :3] - gpos).max(), np.abs(got["fk"][:, :, 3:] - gmat).max())
        print("world", k, "fk error", err)
        assert err <= FK_TOL, (k, err)


@pytest.mark.parametrize("D", [9, 3])
def test_fk_against_reference_free_base(exe, tmp, cells, D):
    """the frozen slide and the second free body behind a free base; dof = 3 cuts the base"""
    c = cells["base"]
    q = S.arm_poses(D, 300, FK_SEED + D, 2.0, True)
    for k, world in enumerate(c["worlds"]):
        got = WH.run(exe, c["xml"], D, WH.world_ops(c["m"]["body_names"], world), q, tmp, tag="bfk%d" % k)
        m, w = ref_of(c, world)
        gpos, gmat = WR.fk(m, w, q, D)
        err = max(np.abs(got["fk"][:, :, :3] - gpos).max(), np.abs(got["fk"][:, :, 3:] - gmat).max())
        assert err <= FK_TOL, (k, err)


def test_contacts_against_reference(exe, tmp, cells):
    c = cells["cell"]
    q = WS.cell_poses(5, 2000, CONTACT_SEED)
    rows = []
    for k, world in enumerate(c["worlds"]):
        got = WH.run(exe, c["xml"], 5, WH.world_ops(c["m"]["body_names"], world), q, tmp, tag="ct%d" % k)
        m, w = ref_of(c, world)
        hit, near, per_pair = WR.contacts(m, 5, w, q)
        assert not near.any(), (k, int(near.sum()))  # (the seed: no decisive distance near its margin)
        mv, _ = R.pairs(m, 5)
        assert [(p[0], p[1]) for p in got["pairs"]] == [(g1, g2) for g1, g2, _ in mv]
        np.testing.assert_array_equal(got["hit"].astype(bool), hit)
        np.testing.assert_array_equal(got["contact"] > 0, per_pair)
        np.testing.assert_array_equal(got["first"], np.where(per_pair.any(1), per_pair.argmax(1), -1))
        assert 0.05 < hit.mean() < 0.95
        rows.append(got["hit"])
    assert len({r.tobytes() for r in rows}) == len(rows)  # (the worlds decide differently)


def test_static_contacts(exe, tmp, cells):
    c = cells["cell"]
    q = WS.cell_poses(5, 16, 3)
    rest = WH.run(exe, c["xml"], 5, [], q, tmp, count_static=1, tag="rest")
    up = c["m"]["qpos0"].copy()
    up[8:11] = WS.BLOCK_UP
    lifted = WH.run(exe, c["xml"], 5, [WH.op_qpos(up)], q, tmp, count_static=1, tag="lift")
    back = WH.run(exe, c["xml"], 5, [WH.op_qpos(up), WH.op_qpos(c["m"]["qpos0"])], q, tmp, count_static=1, tag="back")
    assert rest["info"]["static_contacts"] > 0 and lifted["info"]["static_contacts"] == 0
    for o, world in ((rest, dict(qpos=None, poses=[])), (lifted, dict(qpos=up, poses=[]))):
        assert sum(s[3] for s in o["statics"]) == o["info"]["static_contacts"]
        m, w = ref_of(c, world)
        want, near = WR.static_contacts(m, 5, w)
        assert not near
        assert [(s[0], s[1], s[3] > 0) for s in o["statics"]] == want
    assert rest["hit"].all() and not lifted["hit"].all()  # (count_static: the block on the floor blocks every pose)
    assert back["tables"] == rest["tables"] and back["statics"] == rest["statics"] and back["epoch"] == 2


# ------------------------------------------------------------------ refusals
def test_refusals(exe, tmp, cells):
    c = cells["cell"]
    q0, q = c["m"]["qpos0"], WS.cell_poses(5, 4, 3)
    nan, zero = q0.copy(), q0.copy()
    nan[6] = np.nan
    zero[11:15] = 0.0
    inf = q0.copy()
    inf[9] = np.inf
    good = c["worlds"][1]["qpos"]
    nb = len(c["m"]["body_names"])
    ops = [WH.op_qpos(good), WH.op_qpos(q0[:-1]), WH.op_qpos(list(q0) + [0.0]), WH.op_qpos(nan), WH.op_qpos(inf),
           WH.op_qpos(zero), WH.op_body(nb, (0, 0, 0), (1, 0, 0, 0)), WH.op_body(0, (0, 0, 0), (1, 0, 0, 0)),
           WH.op_body(-1, (0, 0, 0), (1, 0, 0, 0)), WH.op_body(1, (0, np.nan, 0), (1, 0, 0, 0)),
           WH.op_body(1, (0, 0, 0), (0, 0, 0, 0))]
    got = WH.run(exe, c["xml"], 5, ops, q, tmp, tag="refuse")
    only = WH.run(exe, c["xml"], 5, ops[:1], q, tmp, tag="only")
    assert got["rc"] == 0 and got["ops"][0][:2] == [0, 1]
    for rc, epoch, h, err in got["ops"][1:]:
        assert rc == -1 and epoch == 1 and h == got["ops"][0][2] and err, (rc, epoch, err)
    assert "nq = 14" in got["ops"][1][3] and "zero quaternion" in got["ops"][5][3] and "out of range" in got["ops"][6][3]
    assert got["tables"] == only["tables"] and got["epoch"] == 1
    np.testing.assert_array_equal(got["qpos"], only["qpos"])


# ------------------------------------------------------------------ sanitizers
def test_under_sanitizers(tmp, tmp_path_factory, cells):
    d = tmp_path_factory.mktemp("chain_world_san")
    why = H.sanitizer_probe(d)
    if why:
        pytest.skip("no sanitizer runtime on this machine: " + why)
    exe_san = str(d / "check_world_san")
    r = WH.build(exe_san, H.SAN_FLAGS)
    assert r.returncode == 0, r.stderr[-4000:]
    c = cells["cell"]
    q = WS.cell_poses(5, 64, 3)
    bad = c["m"]["qpos0"].copy()
    bad[11:15] = 0.0
    for k, world in enumerate(c["worlds"]):
        ops = WH.world_ops(c["m"]["body_names"], world) + [WH.op_qpos(bad), WH.op_body(99, (0, 0, 0), (1, 0, 0, 0))]
        got = WH.run(exe_san, c["xml"], 5, ops, q, tmp, count_static=1, tag="san%d" % k)
        assert got["rc"] == 0 and "runtime error" not in got["stderr"] and "AddressSanitizer" not in got["stderr"]
    b = cells["base"]
    got = WH.run(exe_san, b["xml"], 3, WH.world_ops(b["m"]["body_names"], b["worlds"][1]), S.arm_poses(3, 64, 4, 2.0, True),
                 tmp, tag="sanb")
    assert got["rc"] == 0 and "runtime error" not in got["stderr"] and "AddressSanitizer" not in got["stderr"]
