"""Python host objects over the C ABI: Model, Scene, SsppJob, TspJob.

Device buffers are torch CUDA tensors (torch is plumbing here: HBM allocation, streams and
torch.distributed); every computation runs in the HIP kernels of libsspp_hip.so.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import (Best, CesBuffers, CesConfig, CesInfo, CesState, ModelView, PairInfo, SceneInfo,
                   SsppArgs, SsppError, TspArgs, check, lib)

DEFAULT_SEED = 0x5EED
SAMPLER_FP64, SAMPLER_FP32 = 0, 1  # sspp_sspp_args::sampler


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(x, n=None):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    if n is not None and a.size != n:
        raise ValueError("expected %d values, got %d" % (n, a.size))
    return a


def _torch():
    import torch  # noqa: WPS433 (plumbing only)
    return torch


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(stream):
    if stream is None:
        torch = _torch()
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)


def _sync(stream):
    torch = _torch()
    if stream is None:
        torch.cuda.current_stream().synchronize()
    elif isinstance(stream, int):
        torch.cuda.synchronize()
    else:
        stream.synchronize()


def best_tensor(device="cuda"):
    """A device buffer for one sspp_best record (4 x int64; cost is the bits of field 0)."""
    return _torch().zeros(4, dtype=_torch().int64, device=device)


def check_records(t):
    """Refuse result records that report lost work: any record (int64 [..., 4] tensor or array)
    whose `reserved` field is non-zero raises SsppError through sspp_best_check
    (SSPP_E_INCOMPLETE).  Returns the records as a numpy int64 [n, 4] array."""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    a = np.ascontiguousarray(a.astype(np.int64).reshape(-1, 4))
    if a.shape[0] and np.any(a[:, 3] != 0):
        check(lib().sspp_best_check(a.ctypes.data_as(C.POINTER(Best)), int(a.shape[0])), "result record")
    return a


def decode_best(t):
    """(cost, index, count) from a best buffer (torch tensor or numpy int64[4]); a record that
    reports lost work raises SsppError (check_records)."""
    a = check_records(t)[0]
    cost = a[:1].view(np.float64)[0]
    return float(cost), int(a[1]), int(a[2])


def reduce_best(parts):
    """Global argmin over gathered per-rank records (cost, index, count[, reserved]): lowest
    cost, lowest id on ties; a record with reserved != 0 raises SsppError."""
    arr = (Best * len(parts))()
    for i, p in enumerate(parts):
        arr[i].cost, arr[i].index, arr[i].count = p[0], p[1], p[2]
        arr[i].reserved = p[3] if len(p) > 3 else 0
    out = Best()
    check(lib().sspp_best_reduce(arr, len(parts), C.byref(out)), "sspp_best_reduce")
    return out.cost, out.index, out.count


def reduce_best_device(parts, out, stream=None):
    """Device argmin over gathered records: parts int64 [n, 4] tensor -> out int64 [4]."""
    n = parts.shape[0]
    check(lib().sspp_best_reduce_device(_ptr(parts), int(n), _ptr(out), _stream(stream)),
          "sspp_best_reduce_device")


class Model:
    """Parsed MJCF scene (SamplingPathPlanner(xml_path) semantics: the string is a path)."""

    def __init__(self, xml_path, joints=False):
        """joints=True also accepts hinge and slide joints (sspp_model_load_mjcf_joints): such a
        model binds to a Chain, not to a Scene."""
        h = C.c_void_p()
        load = lib().sspp_model_load_mjcf_joints if joints else lib().sspp_model_load_mjcf
        check(load(str(xml_path).encode(), C.byref(h)), "load MJCF")
        self._h = h
        self.path = str(xml_path)

    def joints(self):
        """The joints in body pre-order (document order within a body): type (0 free, 2 slide,
        3 hinge), body, qpos address, unit axis and pos in the body frame, names, and qpos0 (a
        hinge's / slide's reference value at its address)."""
        v = _lib.JointView()
        check(lib().sspp_model_joints_get(self._h, C.byref(v)), "model joints")
        nj, nq = v.njnt, v.nq

        def arr(p, n, dt, shape):
            if n == 0:
                return np.zeros(shape, dt)
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt).reshape(shape)

        return dict(
            jnt_type=arr(v.jnt_type, nj, np.int32, (nj,)), jnt_body=arr(v.jnt_body, nj, np.int32, (nj,)),
            jnt_qpos_adr=arr(v.jnt_qpos_adr, nj, np.int32, (nj,)), jnt_axis=arr(v.jnt_axis, 3 * nj, np.float64, (nj, 3)),
            jnt_pos=arr(v.jnt_pos, 3 * nj, np.float64, (nj, 3)), qpos0=arr(v.qpos0, nq, np.float64, (nq,)),
            jnt_names=[(lib().sspp_model_joint_name(self._h, j) or b"").decode() for j in range(nj)],
        )

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None) and _lib._lib is not None:
            _lib._lib.sspp_model_free(self._h)
            self._h = None

    def arrays(self):
        v = ModelView()
        check(lib().sspp_model_view_get(self._h, C.byref(v)), "model view")

        def arr(p, n, dt, shape):
            if n == 0:
                return np.zeros(shape, dt)
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt).reshape(shape)

        nb, ng, ne, nq = v.nbody, v.ngeom, v.nexclude, v.nq
        return dict(
            body_parent=arr(v.body_parent, nb, np.int32, (nb,)),
            body_jnt_type=arr(v.body_jnt_type, nb, np.int32, (nb,)),
            body_qpos_adr=arr(v.body_qpos_adr, nb, np.int32, (nb,)),
            body_pos=arr(v.body_pos, 3 * nb, np.float64, (nb, 3)),
            body_quat=arr(v.body_quat, 4 * nb, np.float64, (nb, 4)),
            geom_type=arr(v.geom_type, ng, np.int32, (ng,)),
            geom_body=arr(v.geom_body, ng, np.int32, (ng,)),
            geom_contype=arr(v.geom_contype, ng, np.int32, (ng,)),
            geom_conaffinity=arr(v.geom_conaffinity, ng, np.int32, (ng,)),
            geom_size=arr(v.geom_size, 3 * ng, np.float64, (ng, 3)),
            geom_pos=arr(v.geom_pos, 3 * ng, np.float64, (ng, 3)),
            geom_quat=arr(v.geom_quat, 4 * ng, np.float64, (ng, 4)),
            geom_margin=arr(v.geom_margin, ng, np.float64, (ng,)),
            exclude=arr(v.exclude, 2 * ne, np.int32, (ne, 2)),
            qpos0=arr(v.qpos0, nq, np.float64, (nq,)),
        )

    def body_id(self, name):
        return check(lib().sspp_model_body_id(self._h, name.encode()), "body lookup")

    def geom_id(self, name):
        return check(lib().sspp_model_geom_id(self._h, name.encode()), "geom lookup")

    def geom_name(self, geom):
        """The geom's name ("" when unnamed): the inverse of geom_id."""
        r = lib().sspp_model_geom_name(self._h, int(geom))
        if r is None:
            raise SsppError("geom id %d out of range" % int(geom))
        return r.decode()

    def body_name(self, body):
        r = lib().sspp_model_body_name(self._h, int(body))
        if r is None:
            raise SsppError("body id %d out of range" % int(body))
        return r.decode()

    def body_point(self, name):
        out = np.zeros(4)
        check(lib().sspp_model_body_point(self._h, name.encode(), _dptr(out)), "body point")
        return out


def _pair_dicts(model, infos, contact=None, deep=None):
    """sspp_pair_info records as dicts (geom ids, names, types, moving flags, margin; with the counts
    of a static-pairs call): Scene's and Chain's pair listings"""
    gt = model.arrays()["geom_type"]
    out = []
    for k, p in enumerate(infos):
        d = dict(geom1=int(p.geom1), geom2=int(p.geom2), name1=model.geom_name(p.geom1),
                 name2=model.geom_name(p.geom2), type1=int(gt[p.geom1]), type2=int(gt[p.geom2]),
                 moving1=bool(p.moving1), moving2=bool(p.moving2), margin=float(p.margin))
        if contact is not None:
            d["contact"], d["deep"] = int(contact[k]), int(deep[k])
        out.append(d)
    return out


class Scene:
    """Model bound to its moving set, with device-resident geom/pair tables.  count_static: the
    SamplingPathPlanner feasibility counts the scene's static-static contacts too (the
    reference's whole-scene ncon, include/sspp.h:143-144; Q7); False ignores them.  The
    TaskSpacePlanner cost always includes them (Collision.h:89-101)."""

    def __init__(self, model, mode, arg, count_static=True):
        if isinstance(arg, str):
            arg = model.body_id(arg)
        h = C.c_void_p()
        check(lib().sspp_scene_create(model.handle, int(mode), int(arg), int(bool(count_static)),
                                      C.byref(h)), "scene create")
        self._h = h
        self.model = model  # keep alive
        self.mode, self.arg = mode, arg

    @property
    def handle(self):
        return self._h

    def info(self):
        i = SceneInfo()
        check(lib().sspp_scene_get_info(self._h, C.byref(i)), "scene info")
        return {k: getattr(i, k) for k, _ in SceneInfo._fields_}

    # Re-posing in place (sspp_scene_set_qpos / _set_body_pose): host-synchronous; no launch that
    # uses the scene may be in flight on the caller's streams.  Every job, planner, executor and
    # CES planner bound to the scene then works in the new world, as fresh objects on a scene
    # loaded with these values would; a captured graph must be captured again.
    def set_qpos(self, qpos):
        """Every free body's pose at once: qpos [nq] in the model's layout (pos, quat each)."""
        q = _f64(qpos)
        check(lib().sspp_scene_set_qpos(self._h, _dptr(q), int(q.size)), "scene set_qpos")

    def set_body_pose(self, body, pos, quat):
        """One body (id or name): a free body's 7 qpos, or a jointless body's pos / quat relative
        to its parent; children follow."""
        if isinstance(body, str):
            body = self.model.body_id(body)
        p, q = _f64(pos, 3), _f64(quat, 4)
        check(lib().sspp_scene_set_body_pose(self._h, int(body), _dptr(p), _dptr(q)), "scene set_body_pose")

    def qpos(self):
        nq = int(self.model.arrays()["qpos0"].size)
        out = np.zeros(nq)
        check(lib().sspp_scene_get_qpos(self._h, _dptr(out), nq), "scene qpos")
        return out

    @property
    def epoch(self):
        v = C.c_int64()
        check(lib().sspp_scene_epoch(self._h, C.byref(v)), "scene epoch")
        return int(v.value)

    # Contact report (sspp_scene_pairs / _static_pairs / _contacts): which geom pairs a pose touches,
    # what the reference reads from mjData.contact[] (Collision::check_collision_point).
    def pairs(self):
        """The moving pairs in report column order: a list of dicts (geom ids, names, types, margin)."""
        n = C.c_int()
        check(lib().sspp_scene_pairs(self._h, None, 0, C.byref(n)), "scene pairs")
        infos = (PairInfo * max(n.value, 1))()
        check(lib().sspp_scene_pairs(self._h, infos, n.value, C.byref(n)), "scene pairs")
        return _pair_dicts(self.model, infos[:n.value])

    def static_pairs(self):
        """The env-env pairs with their `contact` / `deep` counts at the scene's current poses."""
        n = C.c_int()
        check(lib().sspp_scene_static_pairs(self._h, None, None, None, 0, C.byref(n)), "scene static pairs")
        infos = (PairInfo * max(n.value, 1))()
        c, d = (C.c_uint8 * max(n.value, 1))(), (C.c_uint8 * max(n.value, 1))()
        check(lib().sspp_scene_static_pairs(self._h, infos, c, d, n.value, C.byref(n)), "scene static pairs")
        return _pair_dicts(self.model, infos[:n.value], c, d)

    def contacts(self, q, deep=True, stream=None):
        """Per-pair contact counts of N poses: q [N, dof] (MODE_QPOS) or [N, 4] = (x, y, z, yaw)
        (MODE_BODY), a CUDA tensor or an array.  Returns (contact, deep): uint8 tensors [N, P] in
        pairs() column order (deep is None with deep=False).  Synchronises on its stream."""
        torch = _torch()
        D = int(self.arg) if self.mode == _lib.MODE_QPOS else 4
        if not (hasattr(q, "is_cuda") and q.is_cuda):
            q = torch.as_tensor(np.array(q, dtype=np.float64), device="cuda")
        q = q.to(torch.float64).contiguous()
        if q.ndim != 2 or q.shape[1] != D:
            raise SsppError("contacts failed (-1): poses must be [N, %d], got %s" % (D, tuple(q.shape)))
        N, P = int(q.shape[0]), self.info()["n_pairs"]
        c = torch.empty((N, P), dtype=torch.uint8, device=q.device)
        d = torch.empty((N, P), dtype=torch.uint8, device=q.device) if deep else None
        st = _stream(stream)
        check(lib().sspp_scene_contacts(self._h, _ptr(q), N, _ptr(c), _ptr(d), st), "scene contacts")
        _sync(stream)
        return c, d

    def __del__(self):
        if getattr(self, "_h", None) and _lib._lib is not None:
            _lib._lib.sspp_scene_free(self._h)
            self._h = None


class Chain:
    """An articulated model (Model(path, joints=True)) bound to SamplingPathPlanner's pose rule
    q[0:dof] -> qpos[0:dof]: forward kinematics of its driven bodies, contact decisions and spline
    scoring on the device (sspp_chain_*, DESIGN.md §5 "Articulated movers").  count_static: a
    contact among the static geoms makes every pose / candidate infeasible, as for a Scene."""

    def __init__(self, model, dof, count_static=True):
        h = C.c_void_p()
        check(lib().sspp_chain_create(model.handle, int(dof), int(bool(count_static)), C.byref(h)), "chain create")
        self._h = h
        self.model = model  # keep alive
        self.dof = int(dof)

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None) and _lib._lib is not None:
            _lib._lib.sspp_chain_free(self._h)
            self._h = None

    def info(self):
        i = _lib.ChainInfo()
        check(lib().sspp_chain_get_info(self._h, C.byref(i)), "chain info")
        return {k: getattr(i, k) for k, _ in _lib.ChainInfo._fields_}

    def pairs(self):
        """The pair table in evaluation order: dicts of geom ids, names, types, moving flags, margin."""
        n = C.c_int()
        check(lib().sspp_chain_pairs(self._h, None, 0, C.byref(n)), "chain pairs")
        infos = (PairInfo * max(n.value, 1))()
        check(lib().sspp_chain_pairs(self._h, infos, n.value, C.byref(n)), "chain pairs")
        return _pair_dicts(self.model, infos[:n.value])

    def static_pairs(self):
        """The static-static pairs with their `contact` / `deep` counts at the chain's static poses
        (their contacts sum to info()["static_contacts"])."""
        n = C.c_int()
        check(lib().sspp_chain_static_pairs(self._h, None, None, None, 0, C.byref(n)), "chain static pairs")
        infos = (PairInfo * max(n.value, 1))()
        c, d = (C.c_uint8 * max(n.value, 1))(), (C.c_uint8 * max(n.value, 1))()
        check(lib().sspp_chain_static_pairs(self._h, infos, c, d, n.value, C.byref(n)), "chain static pairs")
        return _pair_dicts(self.model, infos[:n.value], c, d)

    # Worlds (sspp_chain_set_qpos / _set_body_pose, DESIGN.md §5 "Worlds for arms"): what the pose
    # rule does not drive.  Host-synchronous; no launch that uses the chain may be in flight on the
    # caller's streams.  Every call afterwards reads the new world; nothing is allocated.
    def set_qpos(self, qpos):
        """The world's qpos [nq] in the model's layout: frozen joints' values, frozen free bodies'
        poses (entries below dof are stored and never read)."""
        q = _f64(qpos)
        check(lib().sspp_chain_set_qpos(self._h, _dptr(q), int(q.size)), "chain set_qpos")

    def set_body_pose(self, body, pos, quat):
        """One body (id or name): a free body's 7 qpos, or any other body's pos / quat relative to
        its parent (a body of the driven chain included); children follow."""
        if isinstance(body, str):
            body = self.model.body_id(body)
        p, q = _f64(pos, 3), _f64(quat, 4)
        check(lib().sspp_chain_set_body_pose(self._h, int(body), _dptr(p), _dptr(q)), "chain set_body_pose")

    def get_qpos(self):
        nq = int(self.model.arrays()["qpos0"].size)
        out = np.zeros(nq)
        check(lib().sspp_chain_get_qpos(self._h, _dptr(out), nq), "chain qpos")
        return out

    @property
    def epoch(self):
        v = C.c_int64()
        check(lib().sspp_chain_epoch(self._h, C.byref(v)), "chain epoch")
        return int(v.value)

    def _worlds(self, worlds, Q):
        """worlds (Q, nq) as a contiguous float64 array"""
        nq = int(self.model.arrays()["qpos0"].size)
        w = np.ascontiguousarray(np.asarray(worlds, dtype=np.float64))
        if w.shape != (Q, nq):
            raise ValueError("worlds must be (%d, %d), got %s" % (Q, nq, w.shape))
        return w

    def _poses(self, q):
        torch = _torch()
        if not (hasattr(q, "is_cuda") and q.is_cuda):
            q = torch.as_tensor(np.array(q, dtype=np.float64), device="cuda")
        q = q.to(torch.float64).contiguous()
        if q.ndim != 2 or q.shape[1] != self.dof:
            raise SsppError("chain failed (-1): poses must be [N, %d], got %s" % (self.dof, tuple(q.shape)))
        return q

    def fk(self, q, stream=None):
        """World poses of every geom at N poses q [N, dof]: (gpos [N, ngeom, 3], gmat [N, ngeom, 9])
        float64 CUDA tensors.  Synchronises on its stream."""
        torch = _torch()
        q = self._poses(q)
        N, ng = int(q.shape[0]), self.info()["n_geoms"]
        gpos = torch.empty((N, ng, 3), dtype=torch.float64, device=q.device)
        gmat = torch.empty((N, ng, 9), dtype=torch.float64, device=q.device)
        check(lib().sspp_chain_fk(self._h, _ptr(q), N, _ptr(gpos), _ptr(gmat), _stream(stream)), "chain fk")
        _sync(stream)
        return gpos, gmat

    def contacts(self, q, stream=None):
        """One byte per pose of q [N, dof]: 1 in contact.  A uint8 CUDA tensor [N]; synchronises."""
        torch = _torch()
        q = self._poses(q)
        N = int(q.shape[0])
        hit = torch.empty((N,), dtype=torch.uint8, device=q.device)
        check(lib().sspp_chain_contacts(self._h, _ptr(q), N, _ptr(hit), _stream(stream)), "chain contacts")
        _sync(stream)
        return hit

    # Contact report (sspp_chain_pair_contacts / _path_contacts / _first_contacts): which pairs a pose
    # or a path touches; columns in pairs() order, static-static pairs left to static_pairs().
    def pair_contacts(self, q, deep=True, stream=None):
        """Per-pair contact counts of N poses q [N, dof] (a CUDA tensor or an array).  Returns
        (contact, deep): uint8 CUDA tensors [N, P] (deep is None with deep=False).  Synchronises on
        its stream."""
        torch = _torch()
        q = self._poses(q)
        N, P = int(q.shape[0]), self.info()["n_pairs"]
        c = torch.empty((N, P), dtype=torch.uint8, device=q.device)
        d = torch.empty((N, P), dtype=torch.uint8, device=q.device) if deep else None
        check(lib().sspp_chain_pair_contacts(self._h, _ptr(q), N, _ptr(c), _ptr(d), _stream(stream)),
              "chain pair_contacts")
        _sync(stream)
        return c, d

    def _splines(self, ctrl):
        torch = _torch()
        if not (hasattr(ctrl, "is_cuda") and ctrl.is_cuda):
            ctrl = torch.as_tensor(np.array(ctrl, dtype=np.float64), device="cuda")
        ctrl = ctrl.to(torch.float64).contiguous()
        if ctrl.ndim != 3 or ctrl.shape[2] != self.dof:
            raise SsppError("chain failed (-1): splines must be [B, n, %d], got %s" % (self.dof, tuple(ctrl.shape)))
        return ctrl

    def path_contacts(self, knots, degree, ctrl, check_points, deep=True, stream=None):
        """Per-pair contact counts of the splines ctrl [B, n, dof] at checkCollision's waypoints
        u = i / check_points, i = 0..check_points (score_ctrl's poses bit for bit).  Returns
        (contact, deep): uint8 CUDA tensors [B, check_points + 1, P].  Synchronises on its stream."""
        torch = _torch()
        knots = _f64(knots)
        ctrl = self._splines(ctrl)
        B, n, W, P = int(ctrl.shape[0]), int(ctrl.shape[1]), int(check_points), self.info()["n_pairs"]
        c = torch.empty((B, W + 1, P), dtype=torch.uint8, device=ctrl.device)
        d = torch.empty((B, W + 1, P), dtype=torch.uint8, device=ctrl.device) if deep else None
        check(lib().sspp_chain_path_contacts(self._h, _dptr(knots), int(degree), _ptr(ctrl), B, n, W, _ptr(c), _ptr(d),
                                             _stream(stream)), "chain path_contacts")
        _sync(stream)
        return c, d

    def first_contacts(self, knots, degree, ctrl, check_points, stream=None):
        """Per spline of ctrl [B, n, dof] its first contact: an int32 CUDA tensor [B, 2] of (lowest
        waypoint in contact, lowest pairs() column in contact there), (-1, -1) for a spline that
        touches nothing.  Static contacts are not counted.  Synchronises on its stream."""
        torch = _torch()
        knots = _f64(knots)
        ctrl = self._splines(ctrl)
        B, n = int(ctrl.shape[0]), int(ctrl.shape[1])
        first = torch.empty((B, 2), dtype=torch.int32, device=ctrl.device)
        check(lib().sspp_chain_first_contacts(self._h, _dptr(knots), int(degree), _ptr(ctrl), B, n, int(check_points),
                                              _ptr(first), _stream(stream)), "chain first_contacts")
        _sync(stream)
        return first

    def score_ctrl(self, knots, degree, ctrl, check_points, first_id, arc, feasible, best, stream=None):
        """checkCollision + computeArcLength + findBestPath on the splines ctrl [B, n, dof] (a CUDA
        tensor) into the caller's device buffers (SsppJob.score_ctrl's contract).  Asynchronous."""
        knots = _f64(knots)
        B, n = int(ctrl.shape[0]), int(ctrl.shape[1])
        check(lib().sspp_chain_score_ctrl(self._h, _dptr(knots), int(degree), _ptr(ctrl), int(first_id), B, n,
                                          int(check_points), _ptr(arc), _ptr(feasible), _ptr(best), _stream(stream)),
              "chain score_ctrl")

    def sample_score(self, knots, degree, init_ctrl, sigma, limits, check_points, first_id, B, arc, feasible, best,
                     ctrl_out=None, seed=DEFAULT_SEED, stream=None):
        """The same on sampleWithNoise's candidates for (seed, ids first_id .. first_id + B)."""
        knots = _f64(knots)
        init = np.ascontiguousarray(np.asarray(init_ctrl, dtype=np.float64))
        n = int(init.shape[0])
        lim = _f64(limits, self.dof)
        check(lib().sspp_chain_sample_score(self._h, _dptr(knots), int(degree), _dptr(init), n, int(check_points),
                                            float(sigma), _dptr(lim), int(seed), int(first_id), int(B), _ptr(arc),
                                            _ptr(feasible), _ptr(ctrl_out), _ptr(best), _stream(stream)),
              "chain sample_score")

    def sample_score_queries(self, knots, degree, init_ctrl, sigma, limits, seeds, check_points, first_id, B, arc,
                             feasible, best=None, ctrl_out=None, best_ctrl=None, stream=None, worlds=None):
        """Q queries in one launch sequence (sspp_chain_sample_score_queries): init_ctrl (Q, n, dof),
        sigma (Q,), limits (Q, dof), seeds (Q,).  Row q of the device tensors arc / feasible (Q, B),
        ctrl_out (Q, B, n, dof), best (Q, 4) and best_ctrl (Q, n, dof, the winner's control points,
        zeros without one) is what sample_score writes for query q alone.  Asynchronous.
        worlds (Q, nq): query q is scored in the chain's world with its qpos replaced by worlds[q]
        (sspp_chain_sample_score_worlds): row q is what sample_score writes after set_qpos(worlds[q])."""
        knots = _f64(knots)
        init_ctrl = np.ascontiguousarray(np.asarray(init_ctrl, dtype=np.float64))
        if init_ctrl.ndim != 3 or init_ctrl.shape[2] != self.dof:
            raise ValueError("init_ctrl must be (Q, n, %d), got %s" % (self.dof, init_ctrl.shape))
        Q, n = int(init_ctrl.shape[0]), int(init_ctrl.shape[1])
        sigma = _f64(sigma, Q)
        limits = np.ascontiguousarray(np.asarray(limits, dtype=np.float64))
        if limits.shape != (Q, self.dof):
            raise ValueError("limits must be (%d, %d), got %s" % (Q, self.dof, limits.shape))
        seeds = np.ascontiguousarray(np.asarray([int(s) & (2 ** 64 - 1) for s in np.asarray(seeds).reshape(-1)],
                                                dtype=np.uint64))
        if seeds.size != Q:
            raise ValueError("expected %d seeds, got %d" % (Q, seeds.size))
        if worlds is not None:
            w = self._worlds(worlds, Q)
            check(lib().sspp_chain_sample_score_worlds(self._h, _dptr(knots), int(degree), Q, _dptr(init_ctrl), n,
                                                       int(check_points), _dptr(sigma), _dptr(limits),
                                                       seeds.ctypes.data_as(C.POINTER(C.c_uint64)), int(first_id), int(B),
                                                       _ptr(arc), _ptr(feasible), _ptr(ctrl_out), _ptr(best),
                                                       _ptr(best_ctrl), _stream(stream), _dptr(w)),
                  "chain sample_score_worlds")
            return
        check(lib().sspp_chain_sample_score_queries(self._h, _dptr(knots), int(degree), Q, _dptr(init_ctrl), n,
                                                    int(check_points), _dptr(sigma), _dptr(limits),
                                                    seeds.ctypes.data_as(C.POINTER(C.c_uint64)), int(first_id), int(B),
                                                    _ptr(arc), _ptr(feasible), _ptr(ctrl_out), _ptr(best),
                                                    _ptr(best_ctrl), _stream(stream)), "chain sample_score_queries")

    def plan_many(self, starts, ends, sigma, limits, sample_count, check_points, init_points, seeds=None, first_id=0,
                  return_all=False, worlds=None):
        """SamplingPathPlanner::plan for Q queries of this arm in one call (sspp_chain_plan_many_host):
        starts / ends (Q, dof); sigma, limits and the shape are shared; seeds (Q,), DEFAULT_SEED each
        when None.  Returns dict(knots, best = Q tuples (cost, index, count), best_ctrl (Q, n, dof),
        n_feasible (Q,)), with return_all also arc (Q, sample_count) and feasible (Q, sample_count).
        Query q's record and winner row are those of a plan of (starts[q], ends[q], seeds[q]) alone.
        worlds (Q, nq): query q is planned in the chain's world with its qpos replaced by worlds[q]
        (sspp_chain_plan_many_worlds_host): as a plan after set_qpos(worlds[q])."""
        starts = np.ascontiguousarray(np.asarray(starts, dtype=np.float64))
        ends = np.ascontiguousarray(np.asarray(ends, dtype=np.float64))
        if starts.ndim != 2 or starts.shape[1] != self.dof or ends.shape != starts.shape:
            raise ValueError("starts and ends must be (Q, %d), got %s and %s" % (self.dof, starts.shape, ends.shape))
        Q, n, B = int(starts.shape[0]), int(init_points), int(sample_count)
        lim = _f64(limits, self.dof)
        seeds = [DEFAULT_SEED] * Q if seeds is None else list(np.asarray(seeds).reshape(-1))
        seeds = np.ascontiguousarray(np.asarray([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64))
        if seeds.size != Q:
            raise ValueError("expected %d seeds, got %d" % (Q, seeds.size))
        knots = np.zeros(max(n, 0) + 4)
        best = (Best * max(Q, 1))()
        best_ctrl = np.zeros((Q, max(n, 0), self.dof))
        nf = np.zeros(max(Q, 1), dtype=np.int64)
        arc = np.zeros((Q, max(B, 0))) if return_all else None
        feas = np.zeros((Q, max(B, 0)), dtype=np.uint8) if return_all else None
        args = (self._h, Q, _dptr(starts), _dptr(ends), float(sigma), _dptr(lim), B, int(check_points), n,
                seeds.ctypes.data_as(C.POINTER(C.c_uint64)), int(first_id), _dptr(knots), best, _dptr(best_ctrl),
                nf.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(arc) if return_all else None,
                feas.ctypes.data_as(C.POINTER(C.c_uint8)) if return_all else None)
        if worlds is not None:
            w = self._worlds(worlds, Q)
            check(lib().sspp_chain_plan_many_worlds_host(*args, _dptr(w)), "chain plan_many (worlds)")
        else:
            check(lib().sspp_chain_plan_many_host(*args), "chain plan_many")
        out = dict(knots=knots, best=[(float(b.cost), int(b.index), int(b.count)) for b in best[:Q]], best_ctrl=best_ctrl,
                   n_feasible=nf[:Q].copy())
        if return_all:
            out["arc"], out["feasible"] = arc, feas
        return out


def interpolate(pts, degree, u):
    """Eigen SplineFitting::Interpolate (include/sspp.h:95): returns (knots, ctrl [n][D])."""
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64))
    n, D = pts.shape
    u = _f64(u, n)
    knots = np.zeros(n + degree + 1)
    ctrl = np.zeros((n, D))
    check(lib().sspp_interpolate(_dptr(pts), n, D, int(degree), _dptr(u), _dptr(knots),
                                 _dptr(ctrl)), "interpolate")
    return knots, ctrl


def spline_eval(knots, degree, ctrl, u):
    knots = _f64(knots)
    ctrl = np.ascontiguousarray(np.asarray(ctrl, dtype=np.float64))
    D = ctrl.shape[1]
    out = np.zeros(D)
    check(lib().sspp_spline_eval(_dptr(knots), knots.size, int(degree), _dptr(ctrl), D,
                                 float(u), _dptr(out)), "spline eval")
    return out


class _Job:
    _h = None

    def info(self):
        a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
        check(lib().sspp_job_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "job info")
        return dict(lanes_per_candidate=a.value, candidates_per_block=b.value,
                    block_threads=c.value, lds_bytes=d.value)

    def set_option(self, key, value):
        """Explicit launch option (include/sspp_hip.h SSPP_OPT_*; tests and tuning)."""
        check(lib().sspp_job_set_option(self._h, int(key), int(value)), "job set_option")

    def get_option(self, key):
        v = C.c_int64()
        check(lib().sspp_job_get_option(self._h, int(key), C.byref(v)), "job get_option")
        return int(v.value)

    def _path_contacts(self, paths, shape, Wn, deep, stream):
        torch = _torch()
        if not (hasattr(paths, "is_cuda") and paths.is_cuda):
            paths = torch.as_tensor(np.array(paths, dtype=np.float64), device="cuda")
        paths = paths.to(torch.float64).contiguous()
        if paths.ndim != 3 or tuple(paths.shape[1:]) != shape:
            raise SsppError("path_contacts failed (-1): paths must be [B, %d, %d], got %s"
                            % (shape[0], shape[1], tuple(paths.shape)))
        if self.scene is None:
            raise SsppError("path_contacts failed (-3): the job has no scene")
        B, P = int(paths.shape[0]), self.scene.info()["n_pairs"]
        c = torch.empty((B, Wn, P), dtype=torch.uint8, device=paths.device)
        d = torch.empty((B, Wn, P), dtype=torch.uint8, device=paths.device) if deep else None
        check(lib().sspp_job_path_contacts(self._h, _ptr(paths), B, _ptr(c), _ptr(d), _stream(stream)),
              "path_contacts")
        _sync(stream)
        return c, d

    def __del__(self):
        if getattr(self, "_h", None) and _lib._lib is not None:
            _lib._lib.sspp_job_free(self._h)
            self._h = None


class SsppJob(_Job):
    """SamplingPathPlanner::plan's candidate loop on the GPU (include/sspp.h:194-225)."""

    def __init__(self, scene, knots, degree, init_ctrl, sigma, limits, check_points,
                 seed=DEFAULT_SEED, max_batch=4096, arc_all=False, sampler=SAMPLER_FP64):
        """arc_all=False follows the reference: arc length only for collision-free candidates
        (findBestPath scores only successful paths), +inf for the others.  sampler: FP64
        Box-Muller normals (default, as std::normal_distribution<double>) or the opt-in FP32
        quads (SAMPLER_FP32)."""
        init_ctrl = np.ascontiguousarray(np.asarray(init_ctrl, dtype=np.float64))
        n, D = init_ctrl.shape
        self.knots = _f64(knots, n + degree + 1)
        self.init_ctrl = init_ctrl
        self.limits = _f64(limits, D)
        self.n, self.D, self.degree, self.W = n, D, int(degree), int(check_points)
        self.max_batch = int(max_batch)
        a = SsppArgs(knots=_dptr(self.knots), degree=self.degree, init_ctrl=_dptr(init_ctrl),
                     n_ctrl=n, dof=D, sigma=float(sigma), limits=_dptr(self.limits),
                     check_points=self.W, seed=int(seed) & (2 ** 64 - 1), arc_all=int(bool(arc_all)),
                     sampler=int(sampler))
        self.sampler = int(sampler)
        h = C.c_void_p()
        check(lib().sspp_job_create_sspp(scene.handle if scene is not None else None, C.byref(a),
                                         self.max_batch, C.byref(h)), "job create (sspp)")
        self._h = h
        self.scene = scene

    def alloc(self, B, device="cuda", with_ctrl=False):
        torch = _torch()
        out = dict(arc=torch.empty(B, dtype=torch.float64, device=device),
                   feasible=torch.empty(B, dtype=torch.uint8, device=device),
                   best=best_tensor(device))
        if with_ctrl:
            out["ctrl"] = torch.empty((B, self.n, self.D), dtype=torch.float64, device=device)
        return out

    def sample_score(self, first_id, B, arc, feasible, best, ctrl_out=None, stream=None):
        check(lib().sspp_job_sample_score(self._h, int(first_id), int(B), _ptr(arc), _ptr(feasible),
                                          _ptr(ctrl_out), _ptr(best), _stream(stream)),
              "sample_score")

    def update(self, init_ctrl, sigma, limits, seed=DEFAULT_SEED, stream=None):
        """Re-target the job to another query of the same shape (sspp_job_update_sspp)."""
        init_ctrl = np.ascontiguousarray(np.asarray(init_ctrl, dtype=np.float64))
        if init_ctrl.shape != (self.n, self.D):
            raise ValueError("init_ctrl must be (%d, %d), got %s" % (self.n, self.D, init_ctrl.shape))
        limits = _f64(limits, self.D)
        check(lib().sspp_job_update_sspp(self._h, _dptr(init_ctrl), float(sigma), _dptr(limits),
                                         int(seed) & (2 ** 64 - 1), _stream(stream)), "update")

    def set_queries(self, init_ctrl, sigma, limits, seeds, stream=None):
        """A set of Q queries for sample_score_queries (sspp_job_set_queries): init_ctrl
        (Q, n, D), sigma (Q,), limits (Q, D), seeds (Q,).  The job's own query stays as it is."""
        init_ctrl = np.ascontiguousarray(np.asarray(init_ctrl, dtype=np.float64))
        if init_ctrl.ndim != 3 or init_ctrl.shape[1:] != (self.n, self.D):
            raise ValueError("init_ctrl must be (Q, %d, %d), got %s" % (self.n, self.D, init_ctrl.shape))
        Q = init_ctrl.shape[0]
        sigma = _f64(sigma, Q)
        limits = np.ascontiguousarray(np.asarray(limits, dtype=np.float64))
        if limits.shape != (Q, self.D):
            raise ValueError("limits must be (%d, %d), got %s" % (Q, self.D, limits.shape))
        seeds = np.ascontiguousarray(np.asarray([int(s) & (2 ** 64 - 1) for s in np.asarray(seeds).reshape(-1)],
                                                dtype=np.uint64))
        if seeds.size != Q:
            raise ValueError("expected %d seeds, got %d" % (Q, seeds.size))
        check(lib().sspp_job_set_queries(self._h, Q, _dptr(init_ctrl), _dptr(sigma), _dptr(limits),
                                         seeds.ctypes.data_as(C.POINTER(C.c_uint64)), _stream(stream)),
              "set_queries")
        self.n_queries = Q

    def alloc_queries(self, Q, B, device="cuda", with_ctrl=False):
        torch = _torch()
        out = dict(arc=torch.empty((Q, B), dtype=torch.float64, device=device),
                   feasible=torch.empty((Q, B), dtype=torch.uint8, device=device),
                   best=torch.zeros((Q, 4), dtype=torch.int64, device=device))
        if with_ctrl:
            out["ctrl"] = torch.empty((Q, B, self.n, self.D), dtype=torch.float64, device=device)
        return out

    def sample_score_queries(self, first_id, B, arc, feasible, best=None, ctrl_out=None, stream=None):
        """One launch for the whole set: row q of arc / feasible (Q, B), ctrl_out (Q, B, n, D) and
        best (Q, 4) is what update(query q) + sample_score(first_id, B) give."""
        check(lib().sspp_job_sample_score_queries(self._h, int(first_id), int(B), _ptr(arc), _ptr(feasible),
                                                  _ptr(ctrl_out), _ptr(best), _stream(stream)),
              "sample_score_queries")

    def score_ctrl(self, ctrl, first_id, arc, feasible, best, stream=None):
        B = ctrl.shape[0]
        check(lib().sspp_job_score_ctrl(self._h, _ptr(ctrl), int(first_id), int(B), _ptr(arc),
                                        _ptr(feasible), _ptr(best), _stream(stream)), "score_ctrl")

    def path_contacts(self, ctrl, deep=True, stream=None):
        """Per-pair contact counts at every collision waypoint of B splines: ctrl [B, n, D] ->
        (contact, deep) uint8 [B, W + 1, P], waypoint i at u = i / W (sspp_job_path_contacts)."""
        return self._path_contacts(ctrl, (self.n, self.D), self.W + 1, deep, stream)

    def set_shape(self, nt=0, g1=0):
        """Force the k_sspp_c2f launch shape (threads per workgroup 64 / 256, phase-1 lanes per
        candidate); 0, 0 = chosen per launch.  Every shape gives the same results."""
        self.set_option(_lib.OPT_SHAPE_NT, nt)
        self.set_option(_lib.OPT_SHAPE_G1, g1)

    def config(self):
        """The job's effective configuration, read back from the library."""
        g = self.get_option
        return dict(sampler="fp32" if g(_lib.OPT_SAMPLER) else "fp64",
                    shape="%dx%d" % (g(_lib.OPT_LAST_NT), g(_lib.OPT_LAST_G1)),
                    pair_order={0: "scene", 1: "gap", 2: "hit"}[g(_lib.OPT_ORDER)],
                    waypoint_order={0: "bisection", 2: "hit"}[g(_lib.OPT_WP_ORDER)],
                    prepass_ms=g(_lib.OPT_PREPASS_US) / 1e3, sampled_pairs=g(_lib.OPT_NPAIRS),
                    cylinder_box=bool(g(_lib.OPT_CYLBOX)), capsule=bool(g(_lib.OPT_CAPSULE)),
                    cylinder_cylinder=bool(g(_lib.OPT_CYLCYL)),
                    scan="fp32-filtered" if g(_lib.OPT_LAST_F32) else "fp64",
                    split=bool(g(_lib.OPT_LAST_SPLIT)))


class TspJob(_Job):
    """tsp::Planner::plan's evaluation loop on the GPU (include/sspp/tsp_planner.h:89-138)."""

    def __init__(self, scene, start, end, n_vias, check_points, mean=None, sigma=None,
                 lo=(-2, -2, -2, -2), hi=(2, 2, 2, 2), z_min=0.0, w_collision=1.0,
                 seed=DEFAULT_SEED, max_batch=4096, floor=(0.0, 0.01, 10.0)):
        K = int(n_vias)
        self.start, self.end = _f64(start, 4), _f64(end, 4)
        self.mean = _f64(mean if mean is not None else np.zeros((max(K, 1), 4)))
        self.sigma = _f64(sigma if sigma is not None else np.zeros((max(K, 1), 4)))
        self.lo, self.hi = _f64(lo, 4), _f64(hi, 4)
        self.K, self.cp, self.max_batch = K, int(check_points), int(max_batch)
        a = TspArgs(start=_dptr(self.start), end=_dptr(self.end), n_vias=K, check_points=self.cp,
                    w_collision=float(w_collision), mean=_dptr(self.mean), sigma=_dptr(self.sigma),
                    lo=_dptr(self.lo), hi=_dptr(self.hi), z_min=float(z_min),
                    seed=int(seed) & (2 ** 64 - 1), floor_z_min=float(floor[0]),
                    floor_margin=float(floor[1]), floor_scale=float(floor[2]))
        h = C.c_void_p()
        check(lib().sspp_job_create_tsp(scene.handle, C.byref(a), self.max_batch, C.byref(h)),
              "job create (tsp)")
        self._h = h
        self.scene = scene

    def alloc(self, B, device="cuda", with_vias=False):
        torch = _torch()
        f = lambda: torch.empty(B, dtype=torch.float64, device=device)  # noqa: E731
        out = dict(L=f(), Cnf=f(), Cwf=f(), cost=f(),
                   status=torch.empty(B, dtype=torch.uint8, device=device),
                   best=best_tensor(device))
        if with_vias:
            out["vias"] = torch.empty((B, max(self.K, 1), 4), dtype=torch.float64, device=device)
        return out

    def sample_score(self, first_id, B, L, Cnf, Cwf, status, cost, best, vias_out=None, stream=None):
        check(lib().sspp_job_tsp_sample_score(self._h, int(first_id), int(B), _ptr(L), _ptr(Cnf),
                                              _ptr(Cwf), _ptr(status), _ptr(cost), _ptr(vias_out),
                                              _ptr(best), _stream(stream)), "tsp sample_score")

    def score_vias(self, vias, first_id, L, Cnf, Cwf, status, cost, best, stream=None):
        B = vias.shape[0]
        check(lib().sspp_job_tsp_score_vias(self._h, _ptr(vias), int(first_id), int(B), _ptr(L),
                                            _ptr(Cnf), _ptr(Cwf), _ptr(status), _ptr(cost),
                                            _ptr(best), _stream(stream)), "tsp score_vias")

    def path_contacts(self, vias, deep=True, stream=None):
        """Per-pair contact counts at every check point of B via sets: vias [B, K, 4] -> (contact,
        deep) uint8 [B, cp, P], row i - 1 at u = i / cp, i = 1..cp (sspp_job_path_contacts)."""
        return self._path_contacts(vias, (self.K, 4), self.cp, deep, stream)


class SsppSteps:
    """Back-to-back SamplingPathPlanner steps enqueued by the C++ step executor
    (sspp_steps_enqueue_sspp): step i scores ids first_id + i * step_stride + [0, B); steps go
    steps_per_launch to a kernel launch, launch l to branch l % len(jobs) — jobs[b] with
    streams[b] and its scratch arc/feasible buffers (steps_per_launch * B entries each)."""

    def __init__(self, jobs, streams, B, arc_bufs, feas_bufs, steps_per_launch=1):
        nb = len(jobs)
        self._keep = (jobs, streams, arc_bufs, feas_bufs)
        self.arc_bufs, self.feas_bufs = arc_bufs, feas_bufs  # each branch's last launch's outputs
        self._J = (C.c_void_p * nb)(*[j._h for j in jobs])
        self._S = (C.c_void_p * nb)(*[_stream(s).value for s in streams])
        self._A = (C.c_void_p * nb)(*[_ptr(a).value for a in arc_bufs])
        self._F = (C.c_void_p * nb)(*[_ptr(f).value for f in feas_bufs])
        self.nb, self.B, self.spl = nb, int(B), int(steps_per_launch)
        h = C.c_void_p()
        check(lib().sspp_steps_create_sspp(self._J, nb, self._S, self.B, self.spl, self._A, self._F,
                                           C.byref(h)), "steps create")
        self._h = h
        self._run = lib().sspp_steps_run
        self._free = lib().sspp_steps_free

    def enqueue(self, nsteps, first_id, step_stride, best=None):
        """best: None, an (nsteps, 4) int64 device tensor for the per-step argmin records, or
        that tensor's device address as an int (callers in a timed loop cache it)."""
        bp = best if (best is None or isinstance(best, int)) else best.data_ptr()
        rc = self._run(self._h, nsteps, first_id, step_stride, bp)
        if rc:
            check(rc, "steps enqueue")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._free(h)
            self._h = None


class CesPlanner:
    """tsp::Planner's CES iteration on the device (include/sspp/tsp_planner.h:72-145).

    One iteration = begin (reset() or keep the distribution; seed list [mean set, forwarded
    best, samples]) -> eval (k_tsp over the slots) -> update (elites, Distribution::update,
    best, adapt) — all asynchronous on `stream`.  With world > 1 every rank owns
    slots_per_rank consecutive slots: `step` evaluates this rank's slots, all-gathers the
    per-slot results (one RCCL all_gather of a packed f64 record per slot) and runs the same
    update on every rank, so all ranks hold the identical distribution afterwards.

    Arguments follow tsp::TaskSpacePlanner's constructor (include/sspp/tsp.h:12-33); the
    planner's Distribution::z_min is `stddev_initial` as in the reference.
    """

    def __init__(self, scene, stddev_initial=0.3, stddev_min=0.01, stddev_max=0.5,
                 stddev_increase_factor=1.5, stddev_decay_factor=0.95, elite_fraction=0.3,
                 sample_count=50, check_points=50, init_points=3, collision_weight=1.0,
                 z_min=0.0, limits_min=(-2.0,) * 4, limits_max=(2.0,) * 4, sigma_floor=0.0,
                 var_ema_beta=0.2, mean_lr=0.5, floor_margin=0.01, floor_penalty_scale=10.0,
                 seed=DEFAULT_SEED, world=1, rank=0, group=None):
        self.lo, self.hi = _f64(limits_min, 4), _f64(limits_max, 4)
        cfg = CesConfig(samples=int(sample_count), checks=int(check_points),
                        total_points=int(init_points), w_collision=float(collision_weight),
                        elite_fraction=float(elite_fraction), inc=float(stddev_increase_factor),
                        dec=float(stddev_decay_factor), sigma_floor=float(sigma_floor),
                        var_beta=float(var_ema_beta), mean_lr=float(mean_lr),
                        stddev_min=float(stddev_min), stddev_max=float(stddev_max),
                        z_min=float(z_min), dist_z_min=float(stddev_initial), sigma0=0.3,
                        lo=_dptr(self.lo), hi=_dptr(self.hi),
                        # Planner never forwards cfg.z_min/floor_* to its Evaluator
                        floor_z_min=0.0, floor_margin=0.01, floor_scale=10.0,
                        seed=int(seed) & (2 ** 64 - 1))
        self.cfg = cfg
        self.configured_floor = (float(z_min), float(floor_margin), float(floor_penalty_scale))
        h = C.c_void_p()
        check(lib().sspp_ces_create(scene.handle, C.byref(cfg), int(world), C.byref(h)), "ces create")
        self._h = h
        self.scene, self.world, self.rank, self.group = scene, int(world), int(rank), group
        inf = CesInfo()
        check(lib().sspp_ces_get_info(self._h, C.byref(inf)), "ces info")
        self.K, self.n_slots, self.spr = inf.n_vias, inf.n_slots, inf.slots_per_rank
        self.samples = int(sample_count)
        b = CesBuffers()
        check(lib().sspp_ces_get_buffers(self._h, C.byref(b)), "ces buffers")
        self._bufs = b

    def __del__(self):
        if getattr(self, "_h", None) and _lib._lib is not None:
            _lib._lib.sspp_ces_free(self._h)
            self._h = None

    def set_option(self, key, value):
        """Explicit option (SSPP_OPT_CES_FUSED); every setting gives bit-identical iterations."""
        check(lib().sspp_ces_set_option(self._h, int(key), int(value)), "ces set_option")

    def begin(self, start, end, iterate, stream=None):
        self._se = (_f64(start, 4), _f64(end, 4))
        check(lib().sspp_ces_begin(self._h, _dptr(self._se[0]), _dptr(self._se[1]),
                                   int(bool(iterate)), _stream(stream)), "ces begin")

    def eval(self, rank=None, stream=None):
        check(lib().sspp_ces_eval(self._h, self.rank if rank is None else int(rank),
                                  _stream(stream)), "ces eval")

    def update(self, stream=None):
        check(lib().sspp_ces_update(self._h, _stream(stream)), "ces update")

    def step(self, start, end, iterate, stream=None):
        """One plan() iteration on this rank (collective over the group when world > 1)."""
        self.begin(start, end, iterate, stream)
        self.eval(stream=stream)
        if self.world > 1:
            self._exchange(stream)
        self.update(stream)

    def _exchange(self, stream=None):
        """All-gather every rank's slot records (one collective), then unpack them into this
        rank's planner so the update sees the whole candidate list.

        Pack, gather and unpack are all ordered on `stream`: the collective is issued with
        `stream` as torch's current stream (RCCL orders its work after the current stream's
        and makes the current stream wait for the result), so a planner driven on a
        non-default stream cannot gather before the pack or unpack before the gather."""
        torch = _torch()
        rec = 5 + 4 * self.K
        if getattr(self, "_xbuf", None) is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            self._xbuf = (torch.empty(self.spr * rec, dtype=torch.float64, device=dev),
                          torch.empty(self.world * self.spr * rec, dtype=torch.float64, device=dev))
        local, full = self._xbuf
        with torch.cuda.stream(torch_stream(stream)):
            check(lib().sspp_ces_pack(self._h, self.rank, _ptr(local), _stream(stream)), "ces pack")
            all_gather_records(full, local, self.group)
            check(lib().sspp_ces_unpack(self._h, _ptr(full), _stream(stream)), "ces unpack")

    def plan(self, start, end, iterate=False, iterations=1, stream=None):
        """iterations x plan(start, end, iterate) without host synchronisation (world == 1)."""
        if self.world > 1:
            for t in range(int(iterations)):
                self.step(start, end, iterate or t > 0, stream)
            return
        s, e = _f64(start, 4), _f64(end, 4)
        check(lib().sspp_ces_plan(self._h, _dptr(s), _dptr(e), int(bool(iterate)),
                                  int(iterations), _stream(stream)), "ces plan")

    @staticmethod
    def plan_group(planners, starts, ends, iterate=False, iterations=1, stream=None):
        """iterations x plan(start_g, end_g, iterate) of every planner, as one chain of batched
        launches on `stream` (sspp_ces_plan_group: one k_tsp_group per iteration over every
        goal's slots).  Each planner's results equal its own plan(); single-rank planners that
        share the scene, vias, checks, bounds and CES configuration (others run one by one)."""
        pls = list(planners)
        G = len(pls)
        s = _f64(np.asarray(starts, dtype=np.float64).reshape(G, 4), 4 * G)
        e = _f64(np.asarray(ends, dtype=np.float64).reshape(G, 4), 4 * G)
        hs = (C.c_void_p * G)(*[p._h.value for p in pls])
        check(lib().sspp_ces_plan_group(C.cast(hs, C.c_void_p), G, _dptr(s), _dptr(e), int(bool(iterate)), int(iterations),
                                        _stream(stream)), "ces plan group")

    def read(self):
        """Synchronous copy of the last iteration: per-candidate results and the state."""
        st = CesState()
        n, K = self.samples + 2, self.K
        L, Cnf, Cwf, cost = (np.zeros(n) for _ in range(4))
        status = np.zeros(n, np.uint8)
        vias = np.zeros((n, K, 4))
        mean, sigma, lbest = np.zeros((K, 4)), np.zeros((K, 4)), np.zeros((K, 4))
        elites = np.zeros(max(1, n), np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        check(lib().sspp_ces_read(self._h, C.byref(st), p(L), p(Cnf), p(Cwf), p(cost), p(status),
                                  p(vias), p(mean), p(sigma), p(lbest), p(elites)), "ces read")
        m = st.n_candidates
        return dict(n_fixed=st.n_fixed, n_candidates=m, n_success=st.n_success,
                    n_elite=st.n_elite, has_best=bool(st.has_best), best_slot=int(st.best_slot),
                    best_cost=st.best_cost, iteration=int(st.iteration), L=L[:m], C_nf=Cnf[:m],
                    C_wf=Cwf[:m], cost=cost[:m], status=status[:m], vias=vias[:m], mean=mean,
                    sigma=sigma, last_best=lbest, elites=elites[:st.n_elite].copy())

    def set_state(self, mean=None, sigma=None, last_best=None, has_best=-1):
        """Overwrite the device distribution (test / warm-start hook; synchronous)."""
        keep = [None if a is None else _f64(a, 4 * self.K) for a in (mean, sigma, last_best)]
        ptrs = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in keep]
        check(lib().sspp_ces_set_state(self._h, *ptrs, int(has_best)), "ces set_state")


def torch_stream(stream):
    """A torch stream object for `stream` (None = current, raw hipStream_t int = external)."""
    torch = _torch()
    if stream is None:
        return torch.cuda.current_stream()
    if isinstance(stream, int):
        return torch.cuda.ExternalStream(stream)
    return stream


def all_gather_records(out, local, group=None):
    """all_gather_into_tensor of device records on torch's current stream.  RCCL ("nccl")
    gathers device memory directly over xGMI; a gloo group (the CPU tests' backend) is staged
    through host memory, in the same stream order."""
    import torch.distributed as dist
    torch = _torch()
    if dist.get_backend(group) == "gloo":
        host = local.cpu()  # waits for the current stream's work on `local`
        parts = [torch.empty_like(host) for _ in range(dist.get_world_size(group))]
        dist.all_gather(parts, host, group=group)
        out.copy_(torch.stack(parts).view(out.shape))
        return
    dist.all_gather_into_tensor(out, local, group=group)


def reduce_best_steps(parts, out, stream=None):
    """parts: (R, G, 4) int64 device tensor of per-rank step records -> out (G, 4)."""
    R, G = parts.shape[0], parts.shape[1]
    check(lib().sspp_best_reduce_steps(_ptr(parts), int(R), int(G), _ptr(out), _stream(stream)),
          "reduce_best_steps")


def device_count():
    n = C.c_int()
    rc = lib().sspp_device_count(C.byref(n))
    return n.value if rc == 0 else 0


__all__ = ["Model", "Scene", "SsppJob", "TspJob", "CesPlanner", "SsppSteps", "reduce_best_steps", "all_gather_records",
           "torch_stream", "interpolate", "spline_eval", "best_tensor", "check_records",
           "decode_best", "reduce_best", "reduce_best_device", "device_count", "DEFAULT_SEED",
           "SAMPLER_FP64", "SAMPLER_FP32", "math"]
