"""IntersectionVolumeGuide — host-side mirror of the reference guide object (lib/guide.py:11-653) whose arithmetic
runs in libedmp_hip.so (edmp_amd/csrc/guide.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi, franka
from .runtime import get_context, ptr, new_slot_key
from .sdf_terms import TERM, TERMS, default_rows, is_int, span


def row_classes(clearance: np.ndarray, expansion: np.ndarray):
    """Rows with identical (clearance[t], expansion[t]) schedules share one obstacle table: returns
    (row_class (B,) int32, class_clearance (G,T), class_expansion (G,T))."""
    B = clearance.shape[0]
    # a guide owns a contiguous block of rows (infer_serial.py:56-91), so consecutive rows are nearly always equal: compare every
    # row with its predecessor in one vectorised pass and key only the first row of each run (a Python loop over 1024 rows with two
    # tobytes() each cost 1.5 ms per scene - the guide object is rebuilt for every scene, infer_serial.py:112)
    key = np.ascontiguousarray(np.concatenate([clearance, expansion], axis=1)).view(np.uint64)  # bit patterns: -0.0 != 0.0, NaN == NaN
    starts = np.concatenate([[0], 1 + np.flatnonzero(np.any(key[1:] != key[:-1], axis=1))]) if B > 1 else np.array([0])
    keys = {}
    reps = []
    cls_of_run = np.empty(len(starts), dtype=np.int32)
    for j, b in enumerate(starts):
        k = key[b].tobytes()
        if k not in keys:
            keys[k] = len(reps)
            reps.append(int(b))
        cls_of_run[j] = keys[k]
    rc = np.repeat(cls_of_run, np.diff(np.concatenate([starts, [B]]))).astype(np.int32)
    return rc, np.ascontiguousarray(clearance[reps], dtype=np.float64), np.ascontiguousarray(expansion[reps], dtype=np.float64)


def pick_goal(volumes, goals, start, volume_trust_region: float = 0.0008):
    """The reference's IK-goal filter (infer_serial.py:119-129), the host rule stated once: sort the candidates by volume, keep those
    with volume < min + volume_trust_region, take the one nearest to `start` (the first of the sorted list on equal distances: the
    smaller volume, then - the sort is stable - the lower index).  volumes (M,), goals (M, 7), start (7,) -> (index into goals,
    goals[index])."""
    volumes, goals = np.asarray(volumes), np.asarray(goals)
    indices = np.argsort(volumes, kind="stable")
    indices = indices[volumes[indices] < np.min(volumes) + volume_trust_region]
    index = int(indices[np.argmin(np.linalg.norm(start - goals[indices], axis=1))])
    return index, goals[index]


def goal_filter_inputs(n_scenes, starts, goals):
    """SceneBatch.filter_goals' arguments, checked on the host before anything is launched: starts (S, 7) and a list of S arrays
    (M_s, 7), M_s >= 1, all finite -> (starts (S,7) f64, goals (sum M_s, 7) f64 scene after scene, counts (S,) int32)."""
    S = int(n_scenes)
    st = np.ascontiguousarray(np.asarray(starts, dtype=np.float64))
    if st.shape != (S, 7):
        raise ValueError(f"starts must be ({S}, 7), got {st.shape}")
    if isinstance(goals, np.ndarray) and goals.dtype != object:
        goals = list(goals) if goals.ndim == 3 else None
    if goals is None or len(goals) != S:
        raise ValueError(f"goals must be a list of {S} arrays (M_s, 7), one per scene")
    gl = []
    for s, g in enumerate(goals):
        a = np.asarray(g, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 7:
            raise ValueError(f"goals[{s}] must be (M, 7), got {a.shape}")
        if a.shape[0] < 1:
            raise ValueError(f"goals[{s}] is empty: every scene brings at least one candidate")
        if not np.isfinite(a).all():
            raise ValueError(f"goals[{s}] holds non-finite values")
        gl.append(a)
    if not np.isfinite(st).all():
        raise ValueError("starts holds non-finite values")
    return st, np.ascontiguousarray(np.concatenate(gl)), np.asarray([a.shape[0] for a in gl], dtype=np.int32)


def goal_filter_device_inputs(n_scenes, starts, goals, counts):
    """SceneBatch.filter_goals' device form, checked on the host before anything is launched: starts (S, 7) finite; goals a dense
    (sum counts, 7) f64 device tensor, scene after scene; counts (S,), each >= 1 -> (starts (S,7) f64, counts (S,) int32).  The rows
    themselves are not read back: they are what a kernel of this library wrote."""
    S = int(n_scenes)
    st = np.ascontiguousarray(np.asarray(starts, dtype=np.float64))
    if st.shape != (S, 7):
        raise ValueError(f"starts must be ({S}, 7), got {st.shape}")
    if not np.isfinite(st).all():
        raise ValueError("starts holds non-finite values")
    if counts is None:
        raise ValueError("the device form of goals is a dense (sum counts, 7) float64 device tensor together with counts=(S,)")
    cn = np.asarray(counts)
    if cn.shape != (S,) or not np.issubdtype(cn.dtype, np.integer):
        raise ValueError(f"counts must be ({S},) integers, one per scene, got {cn.dtype} {cn.shape}")
    for s in range(S):
        if cn[s] < 1:
            raise ValueError(f"scene {s} brings {int(cn[s])} goal candidates: every scene needs at least one (no IK solution for its target?)")
    if not (isinstance(goals, torch.Tensor) and goals.is_cuda):
        raise ValueError("the device form of goals is a dense (sum counts, 7) float64 device tensor together with counts=(S,)")
    if goals.dtype != torch.float64 or goals.dim() != 2 or tuple(goals.shape) != (int(cn.sum()), 7):
        raise ValueError(f"goals must be a float64 device tensor of shape ({int(cn.sum())}, 7) = (sum counts, 7), got {goals.dtype} {tuple(goals.shape)}")
    return st, np.ascontiguousarray(cn.astype(np.int32))


def goal_pose(target):
    """a goal target - (xyz, quaternion_wxyz) or a (4, 4) / (3, 4) pose - as the checked (3, 4) f64 [R* | p*]; None stays None"""
    from . import ik

    if target is None:
        return None
    if isinstance(target, (tuple, list)) and len(target) == 2 and np.ndim(target[0]) == 1:
        target = ik.pose_matrix(target[0], target[1])
    return ik._check_frame(target, "goal_target")


def sdf_tables(guide_cfgs, batch_size, T, link_half_extents, spheres=None, self_pairs=None):
    """Host tables of the sphere signed-distance guide (edmp_sdf_set), checked before anything touches the device: the sphere table
    (n, 5) f32 [link 0..8, centre xyz in the link-box frame, radius] - ``spheres`` or franka.spheres_from_boxes of the link boxes - and
    the row arrays of ``guide_cfgs`` (``sdf_rows`` (B,), ``sdf_margin`` (B, T), ``smoothness`` (B,); a dict without them gives no SDF
    rows, margin 0 and smoothness 0).  The optional terms (sdf_terms.TERMS), each with its row arrays of ``guide_cfgs`` and the default of
    an absent one, every array finite and >= 0 resp. an integer in its range, a weight > 0 only on an SDF row:
      self-clearance (edmp_sdf_set_self): ``sdf_self_weight`` (B,) and ``sdf_self_margin`` (B, T) (absent: 0), and the (9, 9) link-pair
        mask ``self_pairs`` (None: franka.self_collision_pairs());
      tool-pose goal (edmp_sdf_set_goal): ``sdf_goal_weight`` (B,), ``sdf_goal_rotation`` (B,) and ``sdf_goal_window`` (B,) integers >= 1
        (absent: 0, 0, 8);
      swept clearance (edmp_sdf_set_sweep): ``sdf_sweep_weight`` (B,) and ``sdf_sweep_substeps`` (B,) integers in 2..64 wherever the
        weight is > 0 (absent: 0, 4).
    Returns dict(spheres, rows int32, margin f64, smooth f64, self_weight f64, self_margin f64, self_mask (81,) int32, goal_weight f64,
    goal_rotation f64, goal_window int32, sweep_weight f64, sweep_substeps int32)."""
    B, T = int(batch_size), int(T)
    sph = franka.spheres_from_boxes(link_half_extents) if spheres is None else np.asarray(spheres, dtype=np.float32)
    if sph.ndim != 2 or sph.shape[1] != 5:
        raise ValueError(f"spheres must be (n, 5) = [link, x, y, z, radius], got {sph.shape}")
    if not 1 <= sph.shape[0] <= _capi.MAX_SPHERES:
        raise ValueError(f"{sph.shape[0]} spheres outside 1..{_capi.MAX_SPHERES}")
    if not np.isfinite(sph).all():
        raise ValueError("spheres holds non-finite values")
    if np.any(sph[:, 0] != np.floor(sph[:, 0])) or np.any(sph[:, 0] < 0) or np.any(sph[:, 0] >= franka.N_LINKS):
        raise ValueError(f"spheres: link index outside 0..{franka.N_LINKS - 1}")
    if np.any(sph[:, 4] <= 0):
        raise ValueError("spheres: every radius must be > 0")
    rows = np.asarray(guide_cfgs["sdf_rows"] if "sdf_rows" in guide_cfgs else np.zeros(B))
    margin = np.asarray(guide_cfgs["sdf_margin"] if "sdf_margin" in guide_cfgs else np.zeros((B, T)), dtype=np.float64)
    smooth = np.asarray(guide_cfgs["smoothness"] if "smoothness" in guide_cfgs else np.zeros(B), dtype=np.float64)
    if rows.shape != (B,) or margin.shape != (B, T) or smooth.shape != (B,):
        raise ValueError(f"sdf_rows / sdf_margin / smoothness must be ({B},), ({B}, {T}), ({B},), got {rows.shape}, {margin.shape}, {smooth.shape}")
    if not np.all((rows == 0) | (rows == 1)):
        raise ValueError("sdf_rows: one entry per row, 0 or 1")
    if not (np.isfinite(margin).all() and np.all(margin >= 0) and np.isfinite(smooth).all() and np.all(smooth >= 0)):
        raise ValueError("sdf_margin and smoothness must be finite and >= 0")
    tabs = {}
    for term in TERMS:
        shapes = [(B, T) if k.pair else (B,) for k in term.keys]
        vals = [np.asarray(guide_cfgs[k.cfg] if k.cfg in guide_cfgs else default_rows(k, B, T), **({} if is_int(k) else dict(dtype=np.float64)))
                for k in term.keys]
        if [v.shape for v in vals] != shapes:
            raise ValueError(f"{' / '.join(k.cfg for k in term.keys)} must be {', '.join(map(str, shapes))}, got {', '.join(str(v.shape) for v in vals)}")
        weight = vals[0]
        for k, v in zip(term.keys, vals):
            if not is_int(k):
                bad, must = ~(np.isfinite(v) & (v >= 0)), "finite and >= 0"
            elif not np.issubdtype(v.dtype, np.number):
                bad, must = np.ones(B, dtype=bool), span(k)
            else:
                bad, must = ~((v == np.floor(v)) & (v >= k.lo) & (True if k.hi is None else v <= k.hi)), span(k)
            if k.check == "int_weighted":  # (a row without a weight has nothing that reads the value)
                bad, must = bad & (weight > 0), must + " under a weight > 0"
            if bad.any():
                raise ValueError(f"{k.cfg}: row {int(np.nonzero(bad)[0][0])} holds {v[bad][0]!r}: must be {must}")
        if np.any((weight > 0) & (rows != 1)):
            raise ValueError(f"{term.keys[0].cfg}: row {int(np.nonzero((weight > 0) & (rows != 1))[0][0])} carries a weight > 0 and is not an SDF row")
        tabs[term.name] = {k.hyper: np.ascontiguousarray(v.astype(k.dtype, copy=False)) for k, v in zip(term.keys, vals)}
    extra = dict(self_mask=franka.check_pair_mask(self_pairs))  # what a term takes beside its row arrays (Term.extra), checked last
    out = dict(spheres=np.ascontiguousarray(sph), rows=np.ascontiguousarray(rows.astype(np.int32)), margin=np.ascontiguousarray(margin),
               smooth=np.ascontiguousarray(smooth))
    for term in TERMS:
        out.update(tabs[term.name], **{e: extra[e] for e in term.extra})
    return out


spheres_from_boxes = franka.spheres_from_boxes


def _pair7(start, goal):
    """one start / goal pair as two contiguous (7,) f64 arrays"""
    return [np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(7)) for v in (start, goal)]


def _pairs(n_scenes, starts, goals):
    """the start / goal pairs of a scene batch as two contiguous (S, 7) f64 arrays"""
    out = []
    for name, v in (("starts", starts), ("goals", goals)):
        if v is None:
            raise ValueError(f"{name} is required: ({n_scenes}, 7)")
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
        if a.shape != (n_scenes, 7):
            raise ValueError(f"{name} must be ({n_scenes}, 7), got {a.shape}")
        out.append(a)
    return out


def _term_flag(name):
    """_SlotObject._term_on[name] under the attribute name the flag had before the terms shared one dict: callers that set it keep working"""
    return property(lambda self: self._term_on[name], lambda self, on: self._term_on.__setitem__(name, on))


class _SlotObject:
    """What IntersectionVolumeGuide and SceneBatch share: the resident-slot protocol, and the scoring calls whose single-scene and
    scene-batch entry points differ in their leading dimensions only.  Below, ``shape`` is (B,) for a guide and (S, B) for a batch: the
    shape of every per-row result and, as leading arguments, what tells edmp_x from edmp_scenes_x.  A subclass brings ctx, _slot,
    _upload() (its tables into the current slot), _sdf_host() (make the host sphere table if there is none: True if it did) and
    _set_sdf().  The optional terms of the SDF guide (sdf_terms.TERMS) are handled here once; a subclass brings _term_arrays(name) (the
    term's row arrays in the table's key order), _term_weight(name) (the weights it holds, None if it holds none) and what is its own:
    _self_pairs (the pair mask), _goal_tool,
    _goal_targets ((S, 12) or None = derived), _n_rows and T.  _term_on[name]: the term has been handed over with the sphere table."""

    def _bind(self):
        ctx = self.ctx
        if ctx.bound_guide is self:
            return
        # switch to this object's resident slot; the scene tables / row arrays are rebuilt only if the slot is empty
        have = ctx.lib.edmp_guide_slot(ctx.h, self._slot)
        if have < 0:
            _capi.check(have, "edmp_guide_slot")
        if have != 1:
            ctx.bound_guide = None
            self._upload()
        ctx.bound_guide = self  # only a completely built object counts as bound

    def _bind_sdf(self):
        """_bind for a sphere report: an object built without a sphere table makes its host table first and hands it over once bound"""
        lazy = self._sdf_host()
        self._bind()
        if lazy:  # (a resident slot was bound without its table)
            self._set_sdf()

    def _rows_f64(self, X):
        """a device tensor adopted, anything else uploaded: the contiguous f64 device tensor"""
        if isinstance(X, torch.Tensor) and X.is_cuda:
            return self.ctx.adopt(X.to(torch.float64).contiguous())
        return self.ctx.to_dev(X if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float64), torch.float64)

    def _call(self, single, batch, shape, *args):
        """the entry point `single` for a guide, `batch` for a scene batch"""
        name = batch if len(shape) == 2 else single
        _capi.check(getattr(self.ctx.lib, name)(self.ctx.h, *args), name)

    def _swept(self, Xd, shape, N, pair, want_index):
        """the t = 0 swept volume of every row -> (volumes (rows,) f32 device tensor, arg-min inside each scene (S,) int64 or None)"""
        vols = self.ctx.empty((int(np.prod(shape)),), torch.float32)
        idx = (C.c_int * (shape[0] if len(shape) == 2 else 1))() if want_index else None
        self._call("edmp_row_swept_volumes_dev", "edmp_scenes_swept_volumes_dev", shape, ptr(Xd), *shape, N, _capi.as_pd(pair[0]), _capi.as_pd(pair[1]),
                   ptr(vols), idx)
        return vols, (np.array(idx[:], dtype=np.int64) if want_index else None)

    def _pick(self, Xd, vols, shape, prefer, volume_trust_region):
        """the trust-region pick among the rows of each scene -> (indices (S,) int64, volumes f32, metrics dict of f64, both `shape`d);
        volumes, metrics and the pick stay on the device, the indices come back"""
        from .evaluation import metrics_rows_on, time_rows_on

        ctx = self.ctx
        met = metrics_rows_on(ctx, Xd, return_device=True)
        if prefer == "fastest":  # the duration of the timed motion at the default limits (csrc/timing.hip); NaN for a row that was not timed
            key = time_rows_on(ctx, Xd, return_device=True)["duration"]
        else:
            with torch.cuda.stream(ctx.stream):
                key = met["joint_path_length"] if prefer == "shortest" else torch.neg(met["joint_sparc"])  # SPARC <= 0: closest to 0 = largest
        idx = (C.c_int * (shape[0] if len(shape) == 2 else 1))()
        self._call("edmp_select_row_dev", "edmp_scenes_select_rows_dev", shape, ptr(vols), ptr(key), *shape, C.c_double(float(volume_trust_region)), idx)
        with torch.cuda.stream(ctx.stream):
            m = torch.stack([met[k] for k in met])
        mh = ctx.to_host(m)
        return np.array(idx[:], dtype=np.int64), ctx.to_host(vols).reshape(shape), {k: mh[i].reshape(shape).copy() for i, k in enumerate(met)}

    def _success(self, Xd, shape, N, substeps, return_device):
        """the success dict: per-row arrays `shape`d, the four counts as ints for a guide and as (S,) arrays for a batch"""
        ctx, batch = self.ctx, len(shape) == 2
        flags = ctx.empty((3, int(np.prod(shape))), torch.int32)
        counts = (C.c_int32 * (4 * (shape[0] if batch else 1)))()
        dh = np.ascontiguousarray(franka.dh_table_f64())
        self._call("edmp_success_rows_dev", "edmp_scenes_success_rows_dev", shape, ptr(Xd), *shape, N, int(substeps), _capi.as_pd(dh),
                   C.c_void_p(flags[0].data_ptr()), C.c_void_p(flags[1].data_ptr()), C.c_void_p(flags[2].data_ptr()), counts)
        cn = np.array(counts[:], dtype=np.int64).reshape(-1, 4)
        out = {k: (cn[:, i].copy() if batch else int(cn[0, i])) for i, k in enumerate(("rows_ok", "rows_within", "rows_collision_free", "rows"))}
        if return_device:
            f = flags.view(3, *shape)
            with torch.cuda.stream(ctx.stream):
                cf = f[1] < 0
            ctx.hand_over(cf)  # (a stream-wide wait: it covers cf, enqueued after the synchronisation that brought the counts back, and the flags alike)
            out.update(ok=f[0], first=f[1], within=f[2], collision_free=cf)
        else:
            f = ctx.to_host(flags).reshape(3, *shape)
            out.update(ok=f[0].astype(bool), first=f[1].copy(), within=f[2].astype(bool), collision_free=f[1] < 0)
        return out

    def _self_collision(self, Xd, shape, N, substeps, mask, return_device):
        """the self-collision dict, per-row arrays `shape`d: first, pair (.., 2) with -1 rows, free.  One entry point for a guide and a
        batch: the check reads the robot tables only.  mask: franka.check_pair_mask's (81,) int32."""
        ctx = self.ctx
        out = ctx.empty((2, int(np.prod(shape))), torch.int32)
        dh = np.ascontiguousarray(franka.dh_table_f64())
        _capi.check(ctx.lib.edmp_self_collision_rows_dev(ctx.h, ptr(Xd), int(np.prod(shape)), N, int(substeps), _capi.as_pd(dh), _capi.as_pi32(mask),
                                                         C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr())), "edmp_self_collision_rows_dev")
        if return_device:
            with torch.cuda.stream(ctx.stream):
                first, code = out[0].view(*shape), out[1].view(*shape)
                hit = code >= 0
                pair = torch.where(hit.unsqueeze(-1), torch.stack([code // 9, code % 9], dim=-1), torch.full_like(code, -1).unsqueeze(-1))
                res = {"first": first, "pair": pair.to(torch.int32), "free": ~hit}
            ctx.hand_over(out)  # (the caller's torch ops on the results follow this context's stream)
            return res
        h = ctx.to_host(out)
        first, code = h[0].reshape(shape).copy(), h[1].reshape(shape)
        hit = code >= 0
        pair = np.where(hit[..., None], np.stack([code // 9, code % 9], axis=-1), -1).astype(np.int32)
        return {"first": first, "pair": pair, "free": ~hit}

    def _cost_clearance(self, out, shape):
        """the (2, rows) f64 device output of a report kernel as host arrays of the caller's shape"""
        h = self.ctx.to_host(out)
        return {"cost": h[0].reshape(shape).copy(), "clearance": h[1].reshape(shape).copy()}

    def _sdf_report(self, Xd, shape, W, t, pair):
        """cost and minimum clearance of every row under the sphere model; W = the waypoints per row that the entry point takes"""
        ctx = self.ctx
        out = ctx.empty((2, int(np.prod(shape))), torch.float64)
        self._call("edmp_sdf_rows_dev", "edmp_scenes_sdf_rows_dev", shape, ptr(Xd), *shape, W, int(t), _capi.as_pd(pair[0]), _capi.as_pd(pair[1]),
                   C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()))
        return self._cost_clearance(out, shape)

    def has_term(self, name):
        """some SDF row carries a weight > 0 for the term `name` (sdf_terms.TERM)"""
        w = self._term_weight(name)
        return w is not None and bool((w > 0).any())

    has_self_term = property(lambda self: self.has_term("self"), doc="some SDF row carries a self-clearance weight > 0")
    has_goal_term = property(lambda self: self.has_term("goal"), doc="some SDF row carries a goal weight > 0")
    has_sweep_term = property(lambda self: self.has_term("sweep"), doc="some SDF row carries a swept-clearance weight > 0")

    _self_on, _goal_on, _sweep_on = (_term_flag(t.name) for t in TERMS)

    def _bind_term(self, name):
        """_bind_sdf for a term's report: an object without a weighted row hands the term over once (all weights 0: the gradient paths
        launch what they launched)"""
        self._bind_sdf()
        if not self._term_on[name]:
            self._term_on[name] = True
            self._set_term(name)

    def _set_term(self, name):
        """the term's row arrays (_term_arrays, in the table's key order) and what the object itself brings for it -> its setter"""
        term, ctx, n = TERM[name], self.ctx, self._n_rows
        rows = [(_capi.as_pi32 if is_int(k) else _capi.as_pd)(a) for k, a in zip(term.keys, self._term_arrays(name))]
        if name == "self":
            args = [_capi.as_pi32(self._self_pairs), *rows, n, self.T]
        elif name == "goal":
            tool, tg = np.ascontiguousarray(self._goal_tool.reshape(12)), self._goal_targets
            args = [*rows, _capi.as_pd(tool), None if tg is None else _capi.as_pd(tg), n]
        else:
            args = [*rows, n]
        _capi.check(getattr(ctx.lib, term.setter)(ctx.h, *args), term.setter)

    def _set_terms(self):
        """after a sphere table was set (it dropped the terms): every term that is on, in the table's order"""
        for term in TERMS:
            if self._term_on[term.name]:
                self._set_term(term.name)

    def _self_report(self, Xd, shape, ldw, off, L, t):
        """weighted self cost and minimum self clearance of every row; the L interior waypoints at columns off .. of rows of ldw"""
        ctx = self.ctx
        out = ctx.empty((2, int(np.prod(shape))), torch.float64)
        _capi.check(ctx.lib.edmp_sdf_self_rows_dev(ctx.h, ptr(Xd), int(np.prod(shape)), int(ldw), int(off), int(L), int(t), C.c_void_p(out[0].data_ptr()),
                                                   C.c_void_p(out[1].data_ptr())), "edmp_sdf_self_rows_dev")
        return self._cost_clearance(out, shape)

    def _goal_report(self, Xd, shape, ldw, off, L, t):
        """weighted goal cost, tool distance and angle at the last column and the smallest distance, of every row"""
        ctx = self.ctx
        out = ctx.empty((4, int(np.prod(shape))), torch.float64)
        _capi.check(ctx.lib.edmp_sdf_goal_rows_dev(ctx.h, ptr(Xd), int(np.prod(shape)), int(ldw), int(off), int(L), int(t), *(C.c_void_p(out[i].data_ptr()) for i in range(4))),
                    "edmp_sdf_goal_rows_dev")
        h = ctx.to_host(out)
        return {k: h[i].reshape(shape).copy() for i, k in enumerate(("cost", "distance", "angle", "min_distance"))}

    def _sweep_report(self, Xd, shape, W, t, pair, substeps):
        """weighted sweep cost and the minimum clearance over the interpolants of every row; W as _sdf_report takes it"""
        ctx = self.ctx
        out = ctx.empty((2, int(np.prod(shape))), torch.float64)
        self._call("edmp_sdf_sweep_rows_dev", "edmp_scenes_sdf_sweep_rows_dev", shape, ptr(Xd), *shape, W, int(t), _capi.as_pd(pair[0]), _capi.as_pd(pair[1]),
                   0 if substeps is None else int(substeps), C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()))
        return self._cost_clearance(out, shape)

    def _repair(self, X, Xd, shape, N, pair, iters, substeps, margin, smoothness, step, max_step, rows, return_device):
        """projected descent on the swept SDF cost of the (rows, 7, N) device state Xd (made from the caller's X) -> the repair dict, per-row
        arrays `shape`d.  Always out of place: a device tensor of the caller's is cloned first, the kernel runs in place on the clone."""
        ctx, n = self.ctx, int(np.prod(shape))
        with torch.cuda.stream(ctx.stream):
            if isinstance(X, torch.Tensor) and X.is_cuda:
                Xd = Xd.clone()  # (_rows_f64 hands an f64 contiguous device tensor through as it is)
            rep = torch.full((2, n, 2), float("nan"), dtype=torch.float64, device=ctx.device)  # rows outside `rows` are not written
            its = torch.zeros((n,), dtype=torch.int32, device=ctx.device)
        listed = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
        self._call("edmp_sdf_repair_rows_dev", "edmp_scenes_sdf_repair_rows_dev", shape, ptr(Xd), *shape, N, _capi.as_pd(pair[0]), _capi.as_pd(pair[1]),
                   None if listed is None else _capi.as_pi32(listed), 0 if listed is None else int(listed.shape[0]), int(substeps), int(iters), float(margin),
                   float(smoothness), float(step), float(max_step), C.c_void_p(rep[0].data_ptr()), C.c_void_p(rep[1].data_ptr()), ptr(its))
        keys = ("cost0", "cost", "clearance0", "clearance")
        if return_device:
            out = dict(trajectories=Xd.view(*shape, 7, N), iterations=its.view(*shape))
            out.update({k: rep[i // 2, :, i % 2].view(*shape) for i, k in enumerate(keys)})
            ctx.hand_over(Xd)  # (the caller's torch ops on the results follow this context's stream)
            return out
        h = ctx.to_host(rep)
        out = dict(trajectories=ctx.to_host(Xd).reshape(*shape, 7, N), iterations=ctx.to_host(its).reshape(shape))
        out.update({k: h[i // 2, :, i % 2].reshape(shape).copy() for i, k in enumerate(keys)})
        return out

    def _self_mask(self, self_pairs):
        """the ``self_pairs`` argument of shortcut_rows / blend_rows -> None (no self test: the plain entry points) or the (81,) int32 mask:
        True the guide's own (what its SDF self term uses), anything else through franka.check_pair_mask"""
        if self_pairs is None:
            return None
        if self_pairs is True:
            return np.ascontiguousarray(self._self_pairs, dtype=np.int32).reshape(81)
        if self_pairs is False:
            raise ValueError("self_pairs: None (no self test), True (the guide's own pair mask) or a (9, 9) mask")
        return franka.check_pair_mask(self_pairs)

    def _shortcut(self, X, Xd, shape, N, passes, substeps, min_gain, rows, log_cap, return_device, self_pairs=None):
        """shortcutting under the exact collision check of the (rows, 7, N) device state Xd (made from the caller's X) -> the shortcut dict,
        per-row arrays `shape`d.  Always out of place: a device tensor of the caller's is cloned first, the kernel runs in place on the clone.
        self_pairs not None: the *_self_dev entry points, the dict gains self_rejected and self_pairs."""
        ctx, n, cap = self.ctx, int(np.prod(shape)), int(log_cap)
        mask = self._self_mask(self_pairs)
        with torch.cuda.stream(ctx.stream):
            if isinstance(X, torch.Tensor) and X.is_cuda:
                Xd = Xd.clone()  # (_rows_f64 hands an f64 contiguous device tensor through as it is)
            counts = torch.zeros((2 if mask is None else 3, n), dtype=torch.int32, device=ctx.device)  # rows outside `rows` are not written
            length = torch.full((n, 2), float("nan"), dtype=torch.float64, device=ctx.device)
            spans = torch.full((n, max(cap, 0), 2), -1, dtype=torch.int32, device=ctx.device)
        listed = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
        dh = np.ascontiguousarray(franka.dh_table_f64())
        names = ("edmp_shortcut_rows_dev", "edmp_scenes_shortcut_rows_dev") if mask is None else ("edmp_shortcut_rows_self_dev", "edmp_scenes_shortcut_rows_self_dev")
        extra = () if mask is None else (_capi.as_pi32(mask), C.c_void_p(counts[2].data_ptr()))
        self._call(*names, shape, ptr(Xd), *shape, N, None if listed is None else _capi.as_pi32(listed),
                   0 if listed is None else int(listed.shape[0]), int(substeps), int(passes), float(min_gain), _capi.as_pd(dh), C.c_void_p(counts[0].data_ptr()),
                   C.c_void_p(counts[1].data_ptr()), ptr(length), ptr(spans) if cap > 0 else None, cap, *extra)
        if return_device:
            ctx.hand_over(Xd)  # (the caller's torch ops on the results follow this context's stream)
            out = dict(trajectories=Xd.view(*shape, 7, N), accepted=counts[0].view(*shape), tested=counts[1].view(*shape), length0=length[:, 0].view(*shape),
                       length=length[:, 1].view(*shape), spans=spans.view(*shape, max(cap, 0), 2))
            if mask is not None:
                out.update(self_rejected=counts[2].view(*shape), self_pairs=mask.reshape(9, 9).copy())
            return out
        c, ln = ctx.to_host(counts), ctx.to_host(length)
        out = dict(trajectories=ctx.to_host(Xd).reshape(*shape, 7, N), accepted=c[0].reshape(shape).copy(), tested=c[1].reshape(shape).copy(),
                   length0=ln[:, 0].reshape(shape).copy(), length=ln[:, 1].reshape(shape).copy(), spans=(ctx.to_host(spans) if cap > 0 else np.zeros((n, 0, 2), dtype=np.int32)).reshape(*shape, max(cap, 0), 2))
        if mask is not None:
            out.update(self_rejected=c[2].reshape(shape).copy(), self_pairs=mask.reshape(9, 9).copy())
        return out

    @staticmethod
    def _host_state(trajectories):
        """the state of certify_rows, a HOST-ONLY call: an ndarray, nested lists or a CPU tensor -> the contiguous f64 host array.  A device
        tensor is refused (numpy will not read one): the call has no part in the stream order between a caller's stream and the context's."""
        try:
            return np.ascontiguousarray(trajectories, dtype=np.float64)
        except TypeError as e:
            raise TypeError("certify_rows takes host arrays (an ndarray or a CPU tensor) and returns host arrays; for a device-resident state "
                            "call edmp_certify_rows_dev / edmp_scenes_certify_rows_dev, or copy it to the host first") from e

    def _certify(self, Xd, shape, N, depth, margin, rows):
        """the continuous certificate of the (rows, 7, N) device state Xd -> the certify dict of host arrays, per-row arrays `shape`d.  Rows
        outside `rows` are not written by the library: they keep verdict -1, segment -1, fraction -1, link -1, evaluations 0, undecided 0,
        bound NaN."""
        ctx, n = self.ctx, int(np.prod(shape))
        with torch.cuda.stream(ctx.stream):
            ints = torch.zeros((5, n), dtype=torch.int32, device=ctx.device)  # verdict, segment, link, evaluations, undecided
            ints[:3] = -1
            reals = torch.full((2, n), float("nan"), dtype=torch.float64, device=ctx.device)  # fraction, bound
            reals[0] = -1.0
        listed = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
        dh = np.ascontiguousarray(franka.dh_table_f64())
        radii = np.zeros(63, dtype=np.float64)
        self._call("edmp_certify_rows_dev", "edmp_scenes_certify_rows_dev", shape, ptr(Xd), *shape, N, None if listed is None else _capi.as_pi32(listed),
                   0 if listed is None else int(listed.shape[0]), int(depth), float(margin), _capi.as_pd(dh), C.c_void_p(ints[0].data_ptr()),
                   C.c_void_p(ints[1].data_ptr()), C.c_void_p(reals[0].data_ptr()), C.c_void_p(ints[2].data_ptr()), C.c_void_p(ints[3].data_ptr()),
                   C.c_void_p(ints[4].data_ptr()), C.c_void_p(reals[1].data_ptr()), _capi.as_pd(radii))
        keys_i, keys_r = ("verdict", "segment", "link", "evaluations", "undecided"), ("fraction", "bound")
        extra = dict(radii=radii.reshape(9, 7), depth=int(depth), margin=float(margin))
        hi, hr = ctx.to_host(ints), ctx.to_host(reals)
        return dict({k: hi[i].reshape(shape).copy() for i, k in enumerate(keys_i)}, **{k: hr[i].reshape(shape).copy() for i, k in enumerate(keys_r)}, **extra)

    def _blend(self, Xd, shape, N, deviation, reach, substeps, halvings, vmax, amax, jump, scale, rows, return_device, self_pairs=None):
        """the corner blends of the (rows, 7, N) device state Xd under the exact collision check -> the blend dict, per-row arrays `shape`d.
        Rows outside `rows` are not written by the library: they keep beta 0, code 0, halved 0, tested 0 (an unblended row).  self_pairs
        not None: the *_self_dev entry points, the dict gains self_hits and self_pairs."""
        from .evaluation import blend_arguments

        ctx, n = self.ctx, int(np.prod(shape))
        mask = self._self_mask(self_pairs)
        vm, am, jm = franka.timing_limits(vmax, amax, jump, scale)
        dev, reach, substeps, halvings = blend_arguments(deviation, reach, substeps, halvings)
        with torch.cuda.stream(ctx.stream):
            beta = torch.zeros((n, N), dtype=torch.float64, device=ctx.device)
            codes = torch.zeros((2 if mask is None else 3, n, N), dtype=torch.int32, device=ctx.device)
            tested = torch.zeros((n,), dtype=torch.int32, device=ctx.device)
        listed = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
        dh = np.ascontiguousarray(franka.dh_table_f64())
        names = ("edmp_blend_rows_dev", "edmp_scenes_blend_rows_dev") if mask is None else ("edmp_blend_rows_self_dev", "edmp_scenes_blend_rows_self_dev")
        extra = () if mask is None else (_capi.as_pi32(mask), C.c_void_p(codes[2].data_ptr()))
        self._call(*names, shape, ptr(Xd), *shape, N, None if listed is None else _capi.as_pi32(listed),
                   0 if listed is None else int(listed.shape[0]), _capi.as_pd(vm), _capi.as_pd(am), _capi.as_pd(jm), _capi.as_pd(dev), reach, substeps, halvings,
                   _capi.as_pd(dh), ptr(beta), C.c_void_p(codes[0].data_ptr()), C.c_void_p(codes[1].data_ptr()), ptr(tested), *extra)
        lim = dict(vmax=vm, amax=am, jump=jm, deviation=dev, reach=reach, substeps=substeps, halvings=halvings)
        if return_device:
            for v in (beta, codes, tested):
                ctx.hand_over(v)  # (the caller's torch ops on the results follow this context's stream)
            out = dict(beta=beta.view(*shape, N), code=codes[0].view(*shape, N), halved=codes[1].view(*shape, N), tested=tested.view(*shape), **lim)
            if mask is not None:
                out.update(self_hits=codes[2].view(*shape, N), self_pairs=mask.reshape(9, 9).copy())
            return out
        c = ctx.to_host(codes)
        out = dict(beta=ctx.to_host(beta).reshape(*shape, N), code=c[0].reshape(*shape, N).copy(), halved=c[1].reshape(*shape, N).copy(),
                   tested=ctx.to_host(tested).reshape(shape), **lim)
        if mask is not None:
            out.update(self_hits=c[2].reshape(*shape, N).copy(), self_pairs=mask.reshape(9, 9).copy())
        return out


class IntersectionVolumeGuide(_SlotObject):
    """Same constructor / method signatures as the reference:

        guide = IntersectionVolumeGuide(obstacle_config, device, guide_cfgs, batch_size)
        guide.cost(joint_tensor (n,7,L), t, batch_size=None)              -> (n, L, 9*no) f32 tensor
        guide.swept_volume_cost(joint_tensor, start, goal, t, batch_size=None) -> (n, L+1, 9*no)
        guide.get_gradient(joint_input (B,7,48) ndarray, start, goal, t)  -> (B,7,48) f64 ndarray
        guide.choose_best_trajectory(start, goal, trajectories (B,7,50))  -> (7,50)

    Link boxes: the reference measures the Franka collision meshes of pybullet_data every time a guide is built
    (lib/guide.py:245-282).  Here (franka.resolve_link_extents): ``link_mesh_extents`` (9,3) if given, else the meshes in
    ``mesh_dir``, else pybullet_data's directory when importable, else the placeholder table with one warning per process.

    ``bind`` (default True): upload the scene tables and row arrays at once, as the reference's constructor builds its tensors.
    bind=False builds the host tables only; the object binds at its first use.  A guide that only ever serves as one scene of a
    SceneBatch never touches the device on its own.

    The sphere signed-distance guide (csrc/sdf.hip; no counterpart in the reference's live path): rows that ``guide_cfgs["sdf_rows"]``
    marks (guide_cfg.build_guide_cfgs, ``guidance_method: 'sdf'``) take their gradient from the clearance of a sphere model of the arm
    to the TRUE obstacles - oriented boxes, and cylinders where ``obstacle_kinds`` says so (without kinds everything is a cuboid) - plus
    an optional smoothness pull.  ``spheres`` (n, 5) [link 0..8, centre in the link-box frame, radius] replaces the default
    franka.spheres_from_boxes of the link boxes.  get_gradient and the samplers need nothing else: the SDF rows' gradient is overlaid
    below them.  sdf_rows(...) reports cost and minimum clearance of every row.

    Its self-clearance term: SDF rows with ``guide_cfgs["sdf_self_weight"]`` > 0 (guide_cfg: ``hyperparameters.sdf.self_weight``) are also
    pushed away from themselves - the spheres of the link pairs that ``self_pairs`` masks ((9, 9), default
    franka.self_collision_pairs()) are kept ``sdf_self_margin`` apart.  sdf_self_rows(...) reports the term's cost and the minimum self
    clearance of every row.

    Its tool-pose goal term: SDF rows with ``guide_cfgs["sdf_goal_weight"]`` > 0 (guide_cfg: ``hyperparameters.sdf.goal_weight``) are also
    pulled, over their last ``sdf_goal_window`` waypoints, towards the pose ``goal_target`` - (xyz, quaternion_wxyz) or a (4, 4) / (3, 4)
    pose of the tool frame ``goal_tool`` (whatever ik.tool_frame takes) in the base frame; None: the pose of the goal configuration of
    each call.  ``sdf_goal_rotation`` weighs the orientation part.  sdf_goal_rows(...) reports the term's cost and every row's tool
    distance and angle to the target.

    Its swept-clearance term: SDF rows with ``guide_cfgs["sdf_sweep_weight"]`` > 0 (guide_cfg: ``hyperparameters.sdf.sweep_weight``) also
    pay the obstacle hinge at the ``sdf_sweep_substeps`` - 1 joint-space interpolants of every segment of start, waypoints, goal: the
    configurations the success check tests between the waypoints.  sdf_sweep_rows(...) reports the term's cost and every row's minimum
    clearance over those interpolants.

    After the loop: repair_rows(...) moves finished rows by projected descent on the same sphere model's hinge at the waypoints and those
    interpolants (csrc/sdf.hip: sdf_repair_kernel), on any guide - it brings its own scalars and needs no SDF rows.
    """

    def __init__(self, obstacle_config, device, guide_cfgs, batch_size, *, link_mesh_extents=None, mesh_dir=None, obstacle_kinds=None, bind=True,
                 spheres=None, self_pairs=None, goal_target=None, goal_tool=None):
        self.ctx = get_context(device)
        self.device = self.ctx.device
        self.guide_cfgs = guide_cfgs
        self.obstacle_config = np.ascontiguousarray(np.array(obstacle_config, dtype=np.float64))
        if self.obstacle_config.ndim != 2 or self.obstacle_config.shape[1] != 10:
            raise ValueError("obstacle_config must be (n_obstacles, 10) = [xyz, quat xyzw, dims]")
        self.batch_size = int(batch_size)
        self.T = int(np.asarray(guide_cfgs["clearance"]).shape[1])
        clr = np.asarray(guide_cfgs["clearance"], dtype=np.float64)
        exp = np.asarray(guide_cfgs["expansion"], dtype=np.float64)
        if clr.shape[0] != self.batch_size:
            raise ValueError(f"guide_cfgs rows ({clr.shape[0]}) != batch_size ({self.batch_size})")
        self.row_class, self._cls_clr, self._cls_exp = row_classes(clr, exp)
        self.link_mesh_extents = franka.resolve_link_extents(link_mesh_extents, mesh_dir)
        self._half = np.ascontiguousarray(franka.link_half_extents(self.link_mesh_extents))
        self.link_dimensions = torch.from_numpy(self._half * 2)
        self._dh = np.ascontiguousarray(franka.dh_table())
        self._sf = np.ascontiguousarray(franka.static_frames())
        self._sched = np.ascontiguousarray(np.asarray(guide_cfgs["guidance_schedule"], dtype=np.float64))
        self._rows_token = None
        self._slot = new_slot_key()
        # 0 cuboid / 1 cylinder per obstacle row: only the success check reads it (the guide itself sees cylinders as
        # (r, r, h) boxes, quirk Q9).  The reference's loader orders obstacle_config cuboids first, then cylinders
        # (datasets/load_test_dataset.py:141-149), so kinds = [0] * num_cuboids + [1] * num_cylinders there.
        self._kinds = None if obstacle_kinds is None else self._check_kinds(obstacle_kinds)
        self._spheres = spheres
        self._self_pairs = franka.check_pair_mask(self_pairs)
        self._sdf = sdf_tables(guide_cfgs, self.batch_size, self.T, self._half, spheres, self._self_pairs.reshape(9, 9)) if ("sdf_rows" in guide_cfgs or spheres is not None) else None
        from . import ik

        self._goal_tool = np.ascontiguousarray(ik.tool_frame(goal_tool))  # (3, 4)
        self._goal_target = goal_pose(goal_target)  # (3, 4), or None = derived from the goal configuration
        # a term with a weighted row is handed over with the sphere table (its report, on the rows' own values, turns it on too)
        self._term_on = {t.name: self.has_term(t.name) for t in TERMS}
        if bind:
            self._bind()

    # ---- binding -----------------------------------------------------------------------------------------------
    def _upload(self):
        ctx = self.ctx
        no = self.obstacle_config.shape[0]
        _capi.check(
            ctx.lib.edmp_scene_set(ctx.h, _capi.as_pd(self.obstacle_config), no, _capi.as_pd(self._cls_clr), _capi.as_pd(self._cls_exp),
                                   self._cls_clr.shape[0], self.T, _capi.as_pf(self._half), _capi.as_pf(self._dh), _capi.as_pf(self._sf)),
            "edmp_scene_set",
        )
        self._rows_token = None
        self._set_rows(self._sched)
        if self._kinds is not None:
            _capi.check(ctx.lib.edmp_scene_set_shapes(ctx.h, _capi.as_pi32(self._kinds), no), "edmp_scene_set_shapes")

    def _check_kinds(self, kinds):
        k = np.ascontiguousarray(np.asarray(kinds, dtype=np.int32).reshape(-1))
        if k.shape[0] != self.obstacle_config.shape[0] or not np.all((k == 0) | (k == 1)):
            raise ValueError("obstacle_kinds: one entry per obstacle, 0 = cuboid, 1 = cylinder")
        return k

    def set_obstacle_kinds(self, kinds):
        """mark obstacle rows as true cylinders (dims = (r, r, h)) for the success check (lib/environment.py:249-268)."""
        self._kinds = self._check_kinds(kinds)
        self._bind()
        _capi.check(self.ctx.lib.edmp_scene_set_shapes(self.ctx.h, _capi.as_pi32(self._kinds), self._kinds.shape[0]), "edmp_scene_set_shapes")

    def _set_rows(self, sched):
        sched = np.ascontiguousarray(np.asarray(sched, dtype=np.float64))
        token = (sched.shape, sched.tobytes())
        if self._rows_token == token:
            return
        ctx = self.ctx
        method = np.ascontiguousarray(np.asarray(self.guide_cfgs["guidance_method"], dtype=np.float32))
        gn = np.ascontiguousarray(np.asarray(self.guide_cfgs["grad_norm"], dtype=np.float64))
        _capi.check(
            ctx.lib.edmp_rows_set(ctx.h, _capi.as_pi32(self.row_class), _capi.as_pf(method), _capi.as_pd(gn), _capi.as_pd(sched), self.batch_size, sched.shape[1]),
            "edmp_rows_set",
        )
        self._rows_token = token
        if self._sdf is not None:  # the SDF table belongs to the rows: edmp_rows_set dropped it
            self._set_sdf()

    @property
    def has_sdf_rows(self):
        return self._sdf is not None and bool(self._sdf["rows"].any())

    _n_rows = property(lambda self: self.batch_size)
    _goal_targets = property(lambda self: None if self._goal_target is None else np.ascontiguousarray(self._goal_target.reshape(1, 12)))

    def _term_arrays(self, name):
        return [self._sdf[k.hyper] for k in TERM[name].keys]

    def _term_weight(self, name):
        return None if self._sdf is None else self._sdf[TERM[name].keys[0].hyper]

    def _set_sdf(self):
        d, ctx = self._sdf, self.ctx
        _capi.check(ctx.lib.edmp_sdf_set(ctx.h, _capi.as_pf(d["spheres"]), int(d["spheres"].shape[0]), _capi.as_pi32(d["rows"]), _capi.as_pd(d["margin"]),
                                         _capi.as_pd(d["smooth"]), self.batch_size, int(d["margin"].shape[1])), "edmp_sdf_set")
        self._set_terms()  # the terms belong to the sphere table: edmp_sdf_set dropped them

    def _sdf_host(self):
        if self._sdf is not None:
            return False
        self._sdf = sdf_tables(self.guide_cfgs, self.batch_size, self.T, self._half, self._spheres, self._self_pairs.reshape(9, 9))
        return True

    # ---- reference API -----------------------------------------------------------------------------------------
    def define_obstacles(self, obstacle_config=None, t=0, batch_size=None):
        """sets self.obs_min / self.obs_max (b, no, 3) like lib/guide.py:118-158 (read back from the device table)."""
        self._bind()
        b = self.batch_size if batch_size is None else int(batch_size)
        if t != 0 and b != self.batch_size:
            raise ValueError("t != 0 needs batch_size == total batch (the reference broadcasts per-row schedules)")
        no = self.obstacle_config.shape[0]
        tabs = {}
        out = np.zeros((b, no, 6), dtype=np.float32)
        for r in range(b):
            cls = int(self.row_class[r]) if t != 0 else 0
            if cls not in tabs:
                buf = np.zeros((no, 6), dtype=np.float32)
                _capi.check(self.ctx.lib.edmp_scene_read_aabbs(self.ctx.h, cls, int(t), _capi.as_pf(buf)))
                tabs[cls] = buf
            out[r] = tabs[cls]
        self.obs_min = torch.from_numpy(out[:, :, :3].copy())
        self.obs_max = torch.from_numpy(out[:, :, 3:].copy())

    def _cost_common(self, joint_tensor, t, batch_size):
        self._bind()
        jt = self.ctx.to_dev(joint_tensor, torch.float32)
        if jt.dim() != 3 or jt.shape[1] != 7:
            raise ValueError(f"joint tensor must be (n, 7, L), got {tuple(jt.shape)}")
        n, L = jt.shape[0], jt.shape[2]
        b = self.batch_size if batch_size is None else int(batch_size)
        if b != n:
            raise ValueError(f"batch_size ({b}) must equal the number of joint rows ({n})")
        use_rows = 0
        if t != 0:
            if n != self.batch_size:
                raise ValueError("t != 0 needs n == total batch (per-row inflation schedules)")
            use_rows = 1
        return jt, n, L, use_rows

    def cost(self, joint_tensor, t, batch_size=None):
        jt, n, L, use_rows = self._cost_common(joint_tensor, t, batch_size)
        no = self.obstacle_config.shape[0]
        vol = self.ctx.empty((n, L, 9 * no), torch.float32)
        _capi.check(self.ctx.lib.edmp_guide_cost_dev(self.ctx.h, ptr(jt), n, L, int(t), use_rows, ptr(vol)), "edmp_guide_cost_dev")
        self.ctx.sync()
        return vol

    def swept_volume_cost(self, joint_tensor, start, goal, t, batch_size=None):
        jt, n, L, use_rows = self._cost_common(joint_tensor, t, batch_size)
        no = self.obstacle_config.shape[0]
        s = np.ascontiguousarray(np.asarray(start.detach().cpu() if isinstance(start, torch.Tensor) else start, dtype=np.float32).reshape(7))
        g = np.ascontiguousarray(np.asarray(goal.detach().cpu() if isinstance(goal, torch.Tensor) else goal, dtype=np.float32).reshape(7))
        vol = self.ctx.empty((n, L + 1, 9 * no), torch.float32)
        _capi.check(self.ctx.lib.edmp_guide_swept_cost_dev(self.ctx.h, ptr(jt), n, L, int(t), use_rows, _capi.as_pf(s), _capi.as_pf(g), ptr(vol)),
                    "edmp_guide_swept_cost_dev")
        self.ctx.sync()
        return vol

    def get_gradient(self, joint_input, start, goal, t):
        self._bind()
        ctx = self.ctx
        ji = ctx.to_dev(np.asarray(joint_input, dtype=np.float64), torch.float64)
        B, L = ji.shape[0], ji.shape[2]
        s, g = _pair7(start, goal)
        out = ctx.empty((B, 7, L), torch.float64)
        _capi.check(ctx.lib.edmp_guide_gradient_dev(ctx.h, ptr(ji), B, L, _capi.as_pd(s), _capi.as_pd(g), int(t), ptr(out), None), "edmp_guide_gradient_dev")
        return ctx.to_host(out)

    def sdf_rows(self, trajectories, start, goal, t=0):
        """Cost and minimum clearance of EVERY row under the sphere signed-distance model (edmp_sdf_rows_dev): trajectories (n, 7, L)
        interior waypoints, f64 (not clipped) -> {"cost": (n,) f64, "clearance": (n,) f64 = min over the padded chain start, waypoints,
        goal and over the spheres of (distance to the nearest obstacle - radius)}.  t = 0: margin 0, any n (the rows' smoothness weights
        only when n is the guide's batch); t >= 1: the rows' own margin at step t, n = the guide's batch.  A guide built without SDF
        rows and without ``spheres`` uses the default sphere model."""
        self._bind_sdf()
        X = self._rows_f64(trajectories)
        if X.dim() != 3 or X.shape[1] != 7:
            raise ValueError(f"trajectories must be (n, 7, L), got {tuple(X.shape)}")
        return self._sdf_report(X, (X.shape[0],), X.shape[2], t, _pair7(start, goal))

    def sdf_self_rows(self, trajectories, t=0):
        """Self-clearance term of EVERY row (edmp_sdf_self_rows_dev): trajectories (n, 7, L) interior waypoints, f64 (not clipped) ->
        {"cost": (n,) f64 = weight * sum of the hinge terms, "clearance": (n,) f64 = min over the waypoints and the masked sphere pairs
        of (centre distance - both radii), +inf when the mask selects no pair}.  t = 0: margin 0, any n (the rows' weights only when n
        is the guide's batch, else weight 1); t >= 1: the rows' own self margin at step t, n = the guide's batch.  Needs no start /
        goal pair and leaves a segmented run running."""
        X = self._rows_f64(trajectories)
        if X.dim() != 3 or X.shape[1] != 7:
            raise ValueError(f"trajectories must be (n, 7, L), got {tuple(X.shape)}")
        self._bind_term("self")
        return self._self_report(X, (X.shape[0],), X.shape[2], 0, X.shape[2], t)

    def sdf_goal_rows(self, trajectories, t=0):
        """Tool-pose goal term of EVERY row (edmp_sdf_goal_rows_dev): trajectories (n, 7, L) interior waypoints, f64 (not clipped) ->
        {"cost": (n,) f64 = the weighted term, "distance": (n,) f64 tool distance to the target [m] and "angle": (n,) f64 rotation angle
        to it [rad], both at the LAST handed column, "min_distance": (n,) f64 the smallest distance over the handed columns}.  Any n at
        t = 0 (the rows' weights, rotations and windows only when n is the guide's batch, else 1, 1 and L); t changes nothing else.
        With ``goal_target=None`` the target is the pose of the goal of the last call that took a start / goal pair (an error before
        any).  Needs no start / goal pair itself and leaves a segmented run running."""
        X = self._rows_f64(trajectories)
        if X.dim() != 3 or X.shape[1] != 7:
            raise ValueError(f"trajectories must be (n, 7, L), got {tuple(X.shape)}")
        self._bind_term("goal")
        return self._goal_report(X, (X.shape[0],), X.shape[2], 0, X.shape[2], t)

    def sdf_sweep_rows(self, trajectories, start, goal, t=0, substeps=None):
        """Swept-clearance term of EVERY row (edmp_sdf_sweep_rows_dev): trajectories (n, 7, L) interior waypoints, f64 (not clipped) ->
        {"cost": (n,) f64 = weight * sum of the hinge terms at the joint-space interpolants of the L + 1 segments of the padded chain
        start, waypoints, goal, "clearance": (n,) f64 = the smallest sphere clearance over those interpolants (+inf for a row without
        one)}.  substeps=None: the rows' own ``sdf_sweep_weight`` and ``sdf_sweep_substeps``, n = the guide's batch (t >= 1: their
        margin at step t).  substeps=K in 2..64: weight 1 and K - 1 interpolants per segment on any n rows, at t = 0 - with the success
        check's ``substeps`` the clearance covers the configurations that check tests between the waypoints.  The pair is kept apart
        from the guide's own: a segmented run goes on running."""
        X = self._rows_f64(trajectories)
        if X.dim() != 3 or X.shape[1] != 7:
            raise ValueError(f"trajectories must be (n, 7, L), got {tuple(X.shape)}")
        if substeps is None:
            self._bind_term("sweep")
        else:
            self._bind_sdf()
        return self._sweep_report(X, (X.shape[0],), X.shape[2], t, _pair7(start, goal), substeps)

    def repair_rows(self, trajectories, start, goal, iters=32, substeps=4, margin=0.02, smoothness=0.5, step=0.02, max_step=0.02, rows=None,
                    return_device=False):
        """Repair finished rows by projected descent on the swept SDF cost (edmp_sdf_repair_rows_dev, one launch for the whole run of every
        row): trajectories (n, 7, N) f64, ndarray or device tensor, the FULL state - its interior columns 1..N-2 are the waypoints, start /
        goal the pinned ends.  Per iteration a row's cost is the obstacle hinge at ``margin`` over the sphere model at every waypoint AND at
        the ``substeps`` - 1 joint-space interpolants of every segment (with the success check's ``substeps`` both look at the same
        configurations) plus ``smoothness`` times the squared segment lengths; every interior element moves by
        -``step`` x gradient, clamped to +-``max_step`` [rad] and to the joint limits.  A row stops as soon as no hinge term is active, or
        after ``iters`` updates; a row that is clear from the start keeps its bits.  Returns dict(trajectories (n, 7, N), cost0 / cost and
        clearance0 / clearance (n,) f64 of the first / last evaluation - clearance = the smallest sphere clearance over all tested
        configurations, start and goal included -, iterations (n,) int32: updates applied, -1 for a row with a non-finite interior element,
        which is left as it is with NaN reports).  ``rows``: the row indices to work on (any order, no duplicates); the others keep their
        bits and report NaN and 0 iterations.  Always out of place: the input is never modified.  The defaults are the values of one CPU
        experiment on three constructed scenes (tests/repair_inputs.py) - illustrative, not tuned.  The self-clearance and goal terms are
        not part of the repaired cost (self_collision_rows stays the check).  A guide built without SDF rows and without ``spheres`` uses
        the default sphere model.  Leaves a segmented run running."""
        X = self._rows_f64(trajectories)
        if X.dim() != 3 or X.shape[1] != 7:
            raise ValueError(f"trajectories must be (n, 7, N), got {tuple(X.shape)}")
        self._bind_sdf()
        return self._repair(trajectories, X, (X.shape[0],), X.shape[2], _pair7(start, goal), iters, substeps, margin, smoothness, step, max_step, rows,
                            return_device)

    def shortcut_rows(self, trajectories, passes=2, substeps=4, min_gain=1e-6, rows=None, log_cap=128, return_device=False, self_pairs=None):
        """Shortcut finished rows under the exact collision check (edmp_shortcut_rows_dev, csrc/shortcut.hip; one launch, one workgroup per
        row for the whole run of the row): trajectories (n, 7, N) f64, ndarray or device tensor, 3 <= N <= 64, columns 0 and N-1 the pinned
        start and goal.  Per pass the spans s = N-1, then (s+1)//2 down to 2, are walked from i = 0: where replacing the waypoints between
        i and j = i + s by points of the joint-space chord x_i -> x_j shortens the joint path by more than ``min_gain`` [rad], the new piece
        is tested with success_rows' own test at exactly the configurations success_rows will test on it - the new waypoints and the
        ``substeps`` - 1 interpolants of each of its segments - and taken if nothing is hit (then i = j, else i + 1).  A pass that accepts
        nothing ends the row; ``passes`` = 0 is a pure report, and more than 1024 passes (EDMP_MAX_SHORTCUT_PASSES, a cap so that a launch
        stays bounded) are refused.  Consequences: the joint path length never grows; columns 0 and N-1 are
        never written; waypoints are convex combinations of waypoints, so ``within`` cannot get worse; every configuration success_rows
        (at the same ``substeps``) tests on the output is either unchanged or was tested, so ``first`` < 0 before implies ``first`` < 0
        after; a colliding row may become free, when its colliding part lies inside an accepted span.  Self-collision: with
        ``self_pairs`` = None (the default) it is NOT part of the test - a joint-space chord can fold the arm, self_collision_rows stays the
        check.  With ``self_pairs`` = True (the guide's own pair mask, what its SDF self term uses) or a (9, 9) 0/1 mask
        (franka.check_pair_mask) a candidate must also keep every masked pair of link boxes apart at the same configurations, by
        self_collision_rows' own test on the bits it forms (edmp_shortcut_rows_self_dev): a row that self_collision_rows(substeps, pairs=mask)
        calls free before is free after, and the dict gains self_rejected (n,) int32 - the tested candidates that the obstacle test passed
        and the self test rejected - and self_pairs, the (9, 9) mask used.  Returns dict(trajectories (n, 7, N), accepted and
        tested (n,) int32 true counts of accepted spans and tested candidates, length0 / length (n,) f64 joint path length before / after
        as an index-order sum, spans (n, log_cap, 2) int32 the first ``log_cap`` accepted (i, j) in order, the rest -1).  A row with a
        non-finite element is left as it is: accepted = -1, NaN lengths.  ``rows``: the row indices to work on (any order, no duplicates);
        the others keep their bits and report 0 and NaN.  Always out of place: the input is never modified.  Leaves a segmented run
        running."""
        X = self._rows_f64(trajectories)
        if X.dim() != 3 or X.shape[1] != 7:
            raise ValueError(f"trajectories must be (n, 7, N), got {tuple(X.shape)}")
        self._bind()
        return self._shortcut(trajectories, X, (X.shape[0],), X.shape[2], passes, substeps, min_gain, rows, log_cap, return_device, self_pairs)

    def certify_rows(self, trajectories, depth=6, margin=0.0, rows=None):
        """Continuous collision certificate of finished rows (edmp_certify_rows_dev, csrc/certify.hip; one launch, one workgroup per row):
        trajectories (n, 7, N) f64, 2 <= N <= 64.  A HOST-ONLY call: trajectories is an ndarray or a CPU tensor (a device tensor is refused
        with a TypeError) and every result is a host array - the C entry point is the interface for a device-resident state.  success_rows tests a list of configurations; this check
        answers for EVERY configuration of the joint-space polyline.  Per (segment, link) an interval of the segment is certified where a
        lower bound g on the distance between the link box and the obstacles at its centre (csrc/clearance.h) exceeds what the box can move
        inside the interval (the motion radii, franka.motion_radii) by more than ``margin`` [m]; otherwise the exact test decides whether
        the centre is a hit, else the interval is halved, down to ``depth`` (0..10) halvings.  Returns dict(verdict (n,) int32: 0 free - a
        proof that no link box touches an obstacle anywhere on the polyline -, 1 hit - an exact collision at the reported configuration -,
        2 undecided at the depth limit, 3 invalid (a non-finite element; nothing evaluated), names in evaluation.CERTIFY_VERDICT_NAMES;
        segment, fraction (dyadic, exact), link: the lexicographically smallest (segment, fraction, link) among the hits (verdict 1) or
        the first undecided intervals (verdict 2), else -1, -1.0, -1; evaluations, undecided (n,) int32 sums over the row's (N - 1) x 9
        items; bound (n,) f64 the minimum of g - reach over the certified intervals, +inf without one: on a verdict-0 row every link box
        keeps more than bound > margin from every obstacle; radii (9, 7) the table used; depth, margin).  Joint limits are not part of it
        (``within`` stays success_rows'), nor is self-collision.  ``rows``: the row indices to work on (any order, no duplicates); the
        others report verdict -1 and NaN bound.  Read only; leaves a segmented run running."""
        host = self._host_state(trajectories)
        if host.ndim != 3 or host.shape[1] != 7:
            raise ValueError(f"trajectories must be (n, 7, N), got {tuple(host.shape)}")
        self._bind()
        return self._certify(self.ctx.to_dev(host, torch.float64), (host.shape[0],), host.shape[2], depth, margin, rows)

    def row_swept_volumes(self, start, goal, trajectories):
        """(B,) f32 t=0 swept volume per row and the argmin (first on ties)."""
        self._bind()
        X = self._rows_f64(trajectories)
        vols, idx = self._swept(X, (X.shape[0],), X.shape[2], _pair7(start, goal), True)
        return self.ctx.to_host(vols), int(idx[0])

    def success_rows(self, trajectories, substeps: int = 4, return_device: bool = False):
        """Geometric success of EVERY row (edmp_success_rows_dev; stands for RobotEnvironment.benchmark_trajectory,
        lib/environment.py:632-680, and the tally of infer_serial.py:94-99,165-168): trajectories (B,7,N) ndarray or device
        tensor -> dict(ok (B,) bool, first (B,) int32 first colliding waypoint or -1, within (B,) bool, collision_free (B,) bool,
        rows_ok, rows_within, rows_collision_free, rows).  ``collision_free`` (= first < 0) is the REFERENCE's success flag: its
        benchmark_trajectory fails a plan on contact only and merely prints when the joint limits are left
        (lib/environment.py:659-661, 672); ``ok`` = collision_free AND within, the stricter flag.  With return_device the per-row
        arrays stay device tensors (ok / first / within int32, collision_free bool)."""
        self._bind()
        X = self._rows_f64(trajectories)
        if X.dim() != 3 or X.shape[1] != 7:
            raise ValueError(f"trajectories must be (B, 7, N), got {tuple(X.shape)}")
        return self._success(X, (X.shape[0],), X.shape[2], substeps, return_device)

    def self_collision_rows(self, trajectories, substeps: int = 4, pairs=None, return_device: bool = False):
        """Exact self-collision check of EVERY row (edmp_self_collision_rows_dev, csrc/selfcol.hip; stands for the `self_collision`
        metric of the reference's evaluation package, mpinets/metrics.py:278-292): trajectories (n, 7, N) ndarray or device tensor, any
        n >= 1 -> dict(first (n,) int32 waypoint index of the first configuration at which a masked pair of link boxes overlaps or -1,
        pair (n, 2) int32 the first such pair (a, b), a < b, in row-major order at that configuration or (-1, -1), free (n,) bool).
        The configurations are success_rows' (``substeps``); ``pairs`` is a (9, 9) 0/1 mask of which a < b is read, default
        franka.self_collision_pairs().  With return_device the arrays stay device tensors."""
        mask = franka.check_pair_mask(pairs)
        self._bind()
        X = self._rows_f64(trajectories)
        if X.dim() != 3 or X.shape[1] != 7:
            raise ValueError(f"trajectories must be (n, 7, N), got {tuple(X.shape)}")
        return self._self_collision(X, (X.shape[0],), X.shape[2], substeps, mask, return_device)

    def metrics_rows(self, trajectories, dt: float = 0.1, return_device: bool = False):
        """evaluation.batch_metrics on this guide's context: path lengths and SPARC of EVERY row (edmp_metrics_rows_dev; stands for
        lib/metrics.py:11-125) -> dict of four (B,) f64 arrays joint_path_length, ee_path_length, joint_sparc, ee_sparc."""
        from .evaluation import metrics_rows_on

        return metrics_rows_on(self.ctx, trajectories, dt, return_device)

    def time_rows(self, trajectories, vmax=None, amax=None, jump=None, scale=(1, 1), return_device: bool = False):
        """evaluation.time_rows on this guide's context: the fastest rest-to-rest motion along every row's polyline under joint velocity,
        acceleration and corner velocity-jump limits (edmp_time_rows_dev, csrc/timing.hip) -> the profile dict.  Reads nothing of the
        scene; leaves a segmented run running."""
        from .evaluation import time_rows_on

        return time_rows_on(self.ctx, trajectories, vmax, amax, jump, scale, return_device)

    def sample_rows(self, trajectories, profile, period, rows=None, max_samples=None, return_device: bool = False):
        """evaluation.sample_rows on this guide's context: the timed motion of the listed rows at a controller period
        (edmp_sample_rows_dev) -> dict(q, qd (R, 7, M), count (R,), t (M,)).  Leaves a segmented run running."""
        from .evaluation import sample_rows_on

        return sample_rows_on(self.ctx, trajectories, profile, period, rows, max_samples, return_device)

    def blend_rows(self, trajectories, deviation=0.01, reach=0.4, substeps=4, halvings=2, vmax=None, amax=None, jump=None, scale=(1, 1), rows=None,
                   return_device: bool = False, self_pairs=None):
        """Choose a parabolic blend for every corner of finished rows under the exact collision check (edmp_blend_rows_dev, csrc/blend.hip;
        one launch, one workgroup per row): trajectories (n, 7, N) f64, ndarray or device tensor, 2 <= N <= 64, are only read.  Corner i is
        replaced by the quadratic Bezier curve from x_i - beta d_{i-1} over x_i to x_i + beta d_i, which a timed motion crosses at constant
        acceleration and with continuous velocity.  Only a corner whose velocity-jump cap binds (J_i^2 < min(V_{i-1}^2, V_i^2)) is blended;
        beta starts at min(``reach``, 4 ``deviation``_j / |Delta_ij|) and is halved up to ``halvings`` times until the blend's ``substeps`` + 1
        configurations u = k / substeps - both ends included - clear the scene's obstacles under success_rows' own test; a beta whose
        acceleration cap is no better than the jump cap ends the corner.  -> dict(beta (n, N) f64, code (n, N) int32 - index into
        evaluation.BLEND_CODE_NAMES: 0 none (an end, a repeated waypoint, no corner), 1 not needed, 2 no gain, 3 blended, 4 blocked -
        halved (n, N) int32, tested (n,) int32 configurations tested) plus the arguments used.  The blend departs from the polyline by at
        most beta |Delta_ij| / 4 <= ``deviation`` [rad, a scalar or one per joint] in joint j.  Self-collision is NOT tested with
        ``self_pairs`` = None (the default).  With ``self_pairs`` = True (the guide's own pair mask) or a (9, 9) 0/1 mask a try must also keep
        every masked pair of link boxes apart at its ``substeps`` + 1 configurations (edmp_blend_rows_self_dev; self_collision_rows' own
        test): the dict gains self_hits (n, N) int32 - the tries of corner i that the obstacle test passed and the self test rejected - and
        self_pairs, the (9, 9) mask used; a corner whose every try is hit, by whichever test, is code 4.  A row with a
        non-finite element is left alone: code -1, beta NaN.  ``rows``: the rows to work on (any order, no duplicates); the others report
        beta 0, code 0: unblended.  The defaults are illustrative, not tuned: 10 mrad, reach 0.4 (at most 0.45), limits of
        franka.timing_limits.  Hand beta to time_blended_rows.  Leaves a segmented run running."""
        X = self._rows_f64(trajectories)
        if X.dim() != 3 or X.shape[1] != 7:
            raise ValueError(f"trajectories must be (n, 7, N), got {tuple(X.shape)}")
        self._bind()
        out = self._blend(X, (X.shape[0],), X.shape[2], deviation, reach, substeps, halvings, vmax, amax, jump, scale, rows, return_device, self_pairs)
        X.record_stream(self.ctx.stream)
        return out

    def time_blended_rows(self, trajectories, beta, vmax=None, amax=None, jump=None, scale=(1, 1), return_device: bool = False):
        """evaluation.time_blended_rows on this guide's context: the fastest rest-to-rest motion along every row's blended path
        (edmp_time_blended_rows_dev, csrc/timing.hip) -> the blended profile dict.  Reads nothing of the scene; leaves a segmented run running."""
        from .evaluation import time_blended_rows_on

        return time_blended_rows_on(self.ctx, trajectories, beta, vmax, amax, jump, scale, return_device)

    def sample_blended_rows(self, trajectories, profile, period, rows=None, max_samples=None, return_device: bool = False):
        """evaluation.sample_blended_rows on this guide's context (edmp_sample_blended_rows_dev) -> dict(q, qd (R, 7, M), count (R,), t (M,)).
        Leaves a segmented run running."""
        from .evaluation import sample_blended_rows_on

        return sample_blended_rows_on(self.ctx, trajectories, profile, period, rows, max_samples, return_device)

    def select_row(self, start, goal, trajectories, prefer=None, volume_trust_region: float = 0.0008):
        """The row choose_best_trajectory returns, as (index, volumes (B,) f32, metrics dict or None).  prefer=None: the reference's
        rule, the first arg-min of the t = 0 swept volume (lib/guide.py:637-653) - row_swept_volumes' index, nothing else is launched.
        prefer="shortest" / "smoothest": the rule of the reference's IK-goal filter (infer_serial.py:119-129) applied to the plans -
        among the rows whose volume lies within `volume_trust_region` of the minimum, the one with the smallest joint path length /
        the joint SPARC closest to 0 (edmp_select_row_dev on edmp_metrics_rows_dev's output; volumes, metrics and the pick stay on the
        device, one index comes back).  prefer="fastest": the same pick with the key = the duration of the row's timed motion at the default
        limits (evaluation.time_rows); a row that was not timed has a non-finite key and is passed over."""
        if prefer is None:
            vols, idx = self.row_swept_volumes(start, goal, trajectories)
            return idx, vols, None
        if prefer not in ("shortest", "smoothest", "fastest"):
            raise ValueError(f"prefer must be None, 'shortest', 'smoothest' or 'fastest', got {prefer!r}")
        self._bind()
        X = self._rows_f64(trajectories)
        vols, _ = self._swept(X, (X.shape[0],), X.shape[2], _pair7(start, goal), False)
        idx, vh, met = self._pick(X, vols, (X.shape[0],), prefer, volume_trust_region)
        return int(idx[0]), vh, met

    def choose_best_trajectory(self, start, goal, trajectories, *, prefer=None, volume_trust_region: float = 0.0008):
        """lib/guide.py:637-653; the keyword `prefer` (an extension, see select_row) breaks the tie among near-minimal rows."""
        idx, _, _ = self.select_row(start, goal, trajectories, prefer=prefer, volume_trust_region=volume_trust_region)
        return trajectories[idx]


def scene_batch_tables(scenes):
    """Host side of a scene batch (edmp_scene_batch_set + ONE edmp_rows_set): ``scenes`` is a list of S dicts with one scene's
    obstacle_config (no, 10), row_class (B,) int32, class clearance / expansion (G, T), method (B,), grad_norm (B,) and
    guidance_schedule (B, T).  Returns the concatenation the C ABI takes: n_obstacles (S,) int32, obstacle_config (sum no, 10),
    n_classes (S,) int32, clearance / expansion (sum G, T), and the S*B row arrays with row_class renumbered across the scenes
    (scene s's classes follow scene s-1's), so that every row of scene s indexes one of scene s's own class schedules.  Scene dicts that
    carry the row arrays of the sphere signed-distance guide - sdf_rows (B,), sdf_margin (B, T), smoothness (B,), all scenes or none - add
    their concatenation (int32, f64, f64: what edmp_scene_batch_set_sdf takes); without them the result is the dict it always was."""
    if not 1 <= len(scenes) <= _capi.MAX_SCENES:
        raise ValueError(f"a scene batch holds 1..{_capi.MAX_SCENES} scenes, got {len(scenes)}")
    B = int(np.asarray(scenes[0]["row_class"]).shape[0])
    T = int(np.asarray(scenes[0]["clearance"]).shape[1])
    cls_off, row_class, n_obs, n_cls = 0, [], [], []
    for s, sc in enumerate(scenes):
        rc = np.asarray(sc["row_class"], dtype=np.int32).reshape(-1)
        G = int(np.asarray(sc["clearance"]).shape[0])
        no = int(np.asarray(sc["obstacle_config"]).shape[0])
        if rc.shape[0] != B:
            raise ValueError(f"scene {s} has {rc.shape[0]} rows, scene 0 has {B}: every scene of a batch has the same rows")
        if np.asarray(sc["clearance"]).shape != (G, T) or np.asarray(sc["expansion"]).shape != (G, T):
            raise ValueError(f"scene {s}: class schedules must be ({G}, {T})")
        if not 1 <= no <= _capi.MAX_OBSTACLES:
            raise ValueError(f"scene {s} has {no} obstacles, outside 1..{_capi.MAX_OBSTACLES}")
        if rc.size and (rc.min() < 0 or rc.max() >= G):
            raise ValueError(f"scene {s}: row classes outside 0..{G - 1}")
        row_class.append(rc + cls_off)
        n_obs.append(no)
        n_cls.append(G)
        cls_off += G

    def cat(key, dtype, shape_tail=()):
        return np.ascontiguousarray(np.concatenate([np.asarray(sc[key], dtype=dtype).reshape((-1,) + shape_tail) for sc in scenes]))

    out = dict(n_obstacles=np.asarray(n_obs, dtype=np.int32), obstacle_config=cat("obstacle_config", np.float64, (10,)),
               n_classes=np.asarray(n_cls, dtype=np.int32), clearance=cat("clearance", np.float64, (T,)), expansion=cat("expansion", np.float64, (T,)),
               row_class=np.ascontiguousarray(np.concatenate(row_class).astype(np.int32)), method=cat("method", np.float32),
               grad_norm=cat("grad_norm", np.float64), guidance_schedule=cat("guidance_schedule", np.float64, (T,)))
    with_sdf = ["sdf_rows" in sc for sc in scenes]
    if any(with_sdf):
        if not all(with_sdf):
            raise ValueError(f"scene {with_sdf.index(False)} carries no sdf_rows: either every scene of a batch brings its SDF row arrays or none does")
        for s, sc in enumerate(scenes):
            shapes = tuple(np.shape(sc[k]) for k in ("sdf_rows", "sdf_margin", "smoothness"))
            if shapes != ((B,), (B, T), (B,)):
                raise ValueError(f"scene {s}: sdf_rows / sdf_margin / smoothness must be ({B},), ({B}, {T}), ({B},), got {shapes}")
        out.update(sdf_rows=cat("sdf_rows", np.int32), sdf_margin=cat("sdf_margin", np.float64, (T,)), smoothness=cat("smoothness", np.float64))
        for term in TERMS:  # a term's row arrays ride along when every scene brings them (its setter takes them)
            if all(term.keys[0].cfg in sc for sc in scenes):
                out.update({k.cfg: cat(k.cfg, k.dtype, (T,) if k.pair else ()) for k in term.keys})
    return out


class SceneBatch(_SlotObject):
    """S per-scene guides (IntersectionVolumeGuide, one context, equal batch_size and T, one robot) as ONE guide object of the
    library: scene s owns rows [s*B, (s+1)*B) of a (S*B, 7, N) run (Diffusion.denoise_guided_scenes).  The per-scene guides stay
    what they were and may be unbound (IntersectionVolumeGuide(..., bind=False)): the batch reads their host tables only and lives in
    its own resident slot, so switching between it and its scenes re-uploads nothing while both stay resident.

    Before the run, filter_goals picks every scene's goal among its IK candidates in one call (the reference's IK-goal filter), so a
    scene group touches the device through this one object from the first call to the last.

    The finished state is scored on the batch itself, one launch per step for all S scenes: row_swept_volumes, select_rows,
    choose_best_trajectories and success_rows take X as (S, B, 7, N) or (S*B, 7, N), ndarray or device tensor (the tensor of
    denoise_guided_scenes(..., return_device=True) is adopted, not copied) and give, scene by scene, exactly what the scene's own
    guide gives for X[s].  The obstacle kinds of the success check are the guides' own at construction (a guide without kinds counts
    as all cuboids); set_obstacle_kinds replaces them.

    SDF rows (guidance_method 'sdf', csrc/sdf.hip): either every scene of the batch has them or none has - a mix is refused.  In the
    driver a mix does not occur: ONE run config, hence one guide_cfgs, serves every scene of a group.  All members carry the same sphere
    table (one robot per batch); the SDF masks, margins and smoothness weights are row arrays like method and grad_norm and may differ
    from scene to scene.  The batch hands them over with edmp_scene_batch_set_sdf, and every scene's SDF rows - and the grad_norm rows
    that share their norm - equal the scene's own serial run bit for bit.  sdf_rows(...) reports cost and minimum clearance of every row
    of the finished state against its own scene.  The self-clearance term takes one pair mask for the batch and the goal term one tool
    frame (members that disagree are refused) and per-scene targets, all explicit or all derived from the scenes' goals; sdf_self_rows(...)
    and sdf_goal_rows(...) report them.  The swept-clearance term's weights and substeps are row arrays like the margins;
    sdf_sweep_rows(...) reports it for all scenes in one launch."""

    def __init__(self, guides):
        guides = list(guides)
        if not 1 <= len(guides) <= _capi.MAX_SCENES:
            raise ValueError(f"a scene batch holds 1..{_capi.MAX_SCENES} scenes, got {len(guides)}")
        g0 = guides[0]
        for k, g in enumerate(guides):
            if not isinstance(g, IntersectionVolumeGuide):
                raise ValueError(f"scene {k} is not an IntersectionVolumeGuide")
            if g.has_sdf_rows != g0.has_sdf_rows:  # (the members' host tables only: nothing is concatenated or bound yet)
                raise ValueError(f"scene {k} has {'' if g.has_sdf_rows else 'no '}SDF rows (guidance_method 'sdf') and scene 0 has {'' if g0.has_sdf_rows else 'no '}"
                                 "SDF rows: either every scene of a batch has them or none has")
            if g.has_sdf_rows and not np.array_equal(g._sdf["spheres"], g0._sdf["spheres"]):
                raise ValueError(f"scene {k}: the sphere table differs from scene 0's (one robot, one sphere table per batch)")
            if g.ctx is not g0.ctx:
                raise ValueError(f"scene {k} lives on another context than scene 0")
            if g.batch_size != g0.batch_size or g.T != g0.T:
                raise ValueError(f"scene {k}: batch_size / T ({g.batch_size}, {g.T}) differ from scene 0's ({g0.batch_size}, {g0.T})")
            for name in ("_half", "_dh", "_sf"):
                if not np.array_equal(getattr(g, name), getattr(g0, name)):
                    raise ValueError(f"scene {k}: link / DH / static-frame tables differ from scene 0's (one robot per batch)")
        self.guides, self.ctx, self.device = guides, g0.ctx, g0.device
        self.n_scenes, self.batch_size, self.T = len(guides), g0.batch_size, g0.T
        sdf = g0.has_sdf_rows
        self.tables = scene_batch_tables([
            dict(obstacle_config=g.obstacle_config, row_class=g.row_class, clearance=g._cls_clr, expansion=g._cls_exp,
                 method=np.asarray(g.guide_cfgs["guidance_method"], dtype=np.float32).reshape(-1),
                 grad_norm=np.asarray(g.guide_cfgs["grad_norm"], dtype=np.float64).reshape(-1), guidance_schedule=g._sched,
                 **(dict(sdf_rows=g._sdf["rows"], sdf_margin=g._sdf["margin"], smoothness=g._sdf["smooth"],
                        **{k.cfg: g._sdf[k.hyper] for t in TERMS for k in t.keys}) if sdf else {})) for g in guides])
        for k, g in enumerate(guides):  # (host tables still: nothing is bound yet)
            if not np.array_equal(g._self_pairs, g0._self_pairs):
                raise ValueError(f"scene {k}: the self-clearance pair mask (self_pairs) differs from scene 0's: a batch takes one mask")
            if not np.array_equal(g._goal_tool, g0._goal_tool):
                raise ValueError(f"scene {k}: the goal term's tool frame (goal_tool) differs from scene 0's: a batch takes one tool frame")
            if (g._goal_target is None) != (g0._goal_target is None):
                raise ValueError(f"scene {k} brings {'no' if g._goal_target is None else 'an explicit'} goal_target and scene 0 "
                                 f"{'none' if g0._goal_target is None else 'an explicit one'}: the targets of a batch are either all explicit or all derived")
        self._goal_tool = g0._goal_tool
        self._goal_targets = None if g0._goal_target is None else np.ascontiguousarray(np.stack([g._goal_target.reshape(12) for g in guides]))
        self._self_pairs = g0._self_pairs
        self._term_on = {t.name: self.has_term(t.name) for t in TERMS}
        self._spheres = g0._sdf["spheres"] if sdf else None  # None: no SDF table is bound (sdf_rows builds one when a report is asked for)
        self._slot = new_slot_key()
        self._kinds = None
        if any(g._kinds is not None for g in guides):
            self._kinds = np.ascontiguousarray(np.concatenate(
                [g._kinds if g._kinds is not None else np.zeros(g.obstacle_config.shape[0], dtype=np.int32) for g in guides]).astype(np.int32))
        self._bind()

    def _upload(self):
        ctx = self.ctx
        tb, g0 = self.tables, self.guides[0]
        _capi.check(
            ctx.lib.edmp_scene_batch_set(ctx.h, self.n_scenes, _capi.as_pi32(tb["n_obstacles"]), _capi.as_pd(tb["obstacle_config"]),
                                         _capi.as_pi32(tb["n_classes"]), _capi.as_pd(tb["clearance"]), _capi.as_pd(tb["expansion"]), self.T,
                                         _capi.as_pf(g0._half), _capi.as_pf(g0._dh), _capi.as_pf(g0._sf)),
            "edmp_scene_batch_set",
        )
        _capi.check(
            ctx.lib.edmp_rows_set(ctx.h, _capi.as_pi32(tb["row_class"]), _capi.as_pf(tb["method"]), _capi.as_pd(tb["grad_norm"]),
                                  _capi.as_pd(tb["guidance_schedule"]), self.n_scenes * self.batch_size, self.T),
            "edmp_rows_set",
        )
        if self._spheres is not None:  # the SDF table belongs to the rows: after edmp_rows_set
            self._set_sdf()
        if self._kinds is not None:
            _capi.check(ctx.lib.edmp_scene_batch_set_shapes(ctx.h, _capi.as_pi32(self._kinds), int(self._kinds.shape[0])), "edmp_scene_batch_set_shapes")

    @property
    def has_sdf_rows(self):
        return "sdf_rows" in self.tables and bool(self.tables["sdf_rows"].any())

    _n_rows = property(lambda self: self.n_scenes * self.batch_size)

    def _term_arrays(self, name):
        return [self.tables[k.cfg] if k.cfg in self.tables else default_rows(k, self._n_rows, self.T) for k in TERM[name].keys]

    def _term_weight(self, name):
        return self.tables.get(TERM[name].keys[0].cfg)

    def _set_sdf(self):
        tb, ctx, B = self.tables, self.ctx, self.batch_size
        if "sdf_rows" not in tb:  # a report on a batch without SDF rows: no row is overlaid; margins / weights where a member brings them
            zero = dict(rows=np.zeros(B, dtype=np.int32), margin=np.zeros((B, self.T)), smooth=np.zeros(B))
            parts = [g._sdf if g._sdf is not None else zero for g in self.guides]
            tb = dict(sdf_rows=np.ascontiguousarray(np.concatenate([p["rows"] for p in parts]).astype(np.int32)),
                      sdf_margin=np.ascontiguousarray(np.concatenate([p["margin"] for p in parts])),
                      smoothness=np.ascontiguousarray(np.concatenate([p["smooth"] for p in parts])))
        rows, margin, smooth = tb["sdf_rows"], tb["sdf_margin"], tb["smoothness"]
        _capi.check(ctx.lib.edmp_scene_batch_set_sdf(ctx.h, _capi.as_pf(self._spheres), int(self._spheres.shape[0]), _capi.as_pi32(rows), _capi.as_pd(margin),
                                                     _capi.as_pd(smooth), self.n_scenes, self.batch_size, self.T), "edmp_scene_batch_set_sdf")
        self._set_terms()

    def _sdf_host(self):
        if self._spheres is not None:
            return False
        g0 = self.guides[0]
        self._spheres = sdf_tables({}, g0.batch_size, g0.T, g0._half, g0._spheres)["spheres"]
        return True

    # ---- before the run: the IK-goal filter of every scene ---------------------------------------------------------------
    def filter_goals(self, starts, goals, volume_trust_region: float = 0.0008, counts=None):
        """The reference's IK-goal filter (infer_serial.py:117-129) for every scene of the batch in one call
        (edmp_scenes_goal_filter_dev): starts (S, 7); goals a list of S arrays (M_s, 7), the scenes' own candidate counts.  Returns
        (indices (S,) inside the scene, chosen (S, 7) f64, volumes: list of S (M_s,) f32 arrays) - per scene pick_goal's answer on that
        scene's t = 0 candidate volumes.  Wrong shapes, an empty scene and non-finite goals or starts raise ValueError before anything
        is launched.

        The device form: goals a dense (sum M_s, 7) f64 device tensor, scene after scene, with `counts` (S,) - what
        ik.solve(..., return_device=True) returns as goals + counts - goes into the filter as it lies, without a host round trip; the
        results are those of the host form on the same numbers.  A scene with a count of 0 raises ValueError naming the scene."""
        flat = None
        if counts is not None or (isinstance(goals, torch.Tensor) and goals.is_cuda):
            st, counts = goal_filter_device_inputs(self.n_scenes, starts, goals, counts)
        else:
            st, flat, counts = goal_filter_inputs(self.n_scenes, starts, goals)
        self._bind()
        ctx, S = self.ctx, self.n_scenes
        gd = ctx.to_dev(flat, torch.float64) if flat is not None else ctx.adopt(goals.contiguous())
        vols = ctx.empty((gd.shape[0],), torch.float32)
        idx = (C.c_int * S)()
        _capi.check(ctx.lib.edmp_scenes_goal_filter_dev(ctx.h, ptr(gd), S, _capi.as_pi32(counts), _capi.as_pd(st), C.c_double(float(volume_trust_region)),
                                                        ptr(vols), None, idx), "edmp_scenes_goal_filter_dev")
        vh = ctx.to_host(vols)
        off = np.concatenate([[0], np.cumsum(counts)])
        indices = np.array(idx[:], dtype=np.int64)
        if flat is None:
            with torch.cuda.stream(ctx.stream):
                picked = gd[torch.as_tensor(off[:-1] + indices, device=gd.device)]
            chosen = ctx.to_host(picked)
            gd.record_stream(ctx.stream)
        else:
            chosen = flat[off[:-1] + indices].copy()
        return indices, chosen, [vh[off[s]:off[s + 1]].copy() for s in range(S)]

    # ---- scoring the finished state of the batch ------------------------------------------------------------------------
    def _check_kinds(self, kinds):
        if isinstance(kinds, (list, tuple)) and len(kinds) and np.ndim(kinds[0]) == 1:
            kinds = np.concatenate([np.asarray(k).reshape(-1) for k in kinds])  # one array per scene
        k = np.ascontiguousarray(np.asarray(kinds, dtype=np.int32).reshape(-1))
        total = int(np.sum(self.tables["n_obstacles"]))
        if k.shape[0] != total or not np.all((k == 0) | (k == 1)):
            raise ValueError(f"obstacle_kinds: one entry per obstacle of the batch ({total}, scene after scene; got {k.shape[0]}), 0 = cuboid, 1 = cylinder")
        return k

    def set_obstacle_kinds(self, kinds):
        """IntersectionVolumeGuide.set_obstacle_kinds for the batch: the kinds of all obstacles, scene after scene (one flat array or
        one array per scene).  Only success_rows reads them; the per-scene guides keep their own."""
        self._kinds = self._check_kinds(kinds)
        self._bind()
        _capi.check(self.ctx.lib.edmp_scene_batch_set_shapes(self.ctx.h, _capi.as_pi32(self._kinds), int(self._kinds.shape[0])), "edmp_scene_batch_set_shapes")

    def _state(self, X):
        """X as (S, B, 7, N) or (S*B, 7, N), ndarray or device tensor -> the contiguous (S*B, 7, N) f64 device tensor (shape checked first)"""
        S, B = self.n_scenes, self.batch_size
        shape = tuple(X.shape) if isinstance(X, torch.Tensor) else np.shape(X)
        if not ((len(shape) == 4 and shape[:3] == (S, B, 7)) or (len(shape) == 3 and shape[:2] == (S * B, 7))):
            raise ValueError(f"trajectories must be ({S}, {B}, 7, N) or ({S * B}, 7, N), got {tuple(shape)}")
        N = int(shape[-1])
        return self._rows_f64(X).reshape(S * B, 7, N), N

    def _volumes(self, starts, goals, X, want_index):
        pair = _pairs(self.n_scenes, starts, goals)
        Xd, N = self._state(X)
        self._bind()
        vols, idx = self._swept(Xd, (self.n_scenes, self.batch_size), N, pair, want_index)
        Xd.record_stream(self.ctx.stream)
        return Xd, vols, idx

    def row_swept_volumes(self, starts, goals, trajectories):
        """per scene what IntersectionVolumeGuide.row_swept_volumes gives: ((S, B) f32 t = 0 swept volumes, (S,) arg-min inside the scene)"""
        _, vols, idx = self._volumes(starts, goals, trajectories, True)
        return self.ctx.to_host(vols).reshape(self.n_scenes, self.batch_size), idx

    def select_rows(self, starts, goals, trajectories, prefer=None, volume_trust_region: float = 0.0008):
        """IntersectionVolumeGuide.select_row for every scene of the batch: (indices (S,) inside the scene, volumes (S, B) f32, metrics
        dict of (S, B) f64 arrays or None).  prefer=None: the first arg-min per scene; "shortest" / "smoothest" / "fastest": the trust-region
        pick (edmp_scenes_select_rows_dev on ONE edmp_metrics_rows_dev - for "fastest" also ONE edmp_time_rows_dev - call over the S*B rows)."""
        if prefer not in (None, "shortest", "smoothest", "fastest"):
            raise ValueError(f"prefer must be None, 'shortest', 'smoothest' or 'fastest', got {prefer!r}")
        ctx, S, B = self.ctx, self.n_scenes, self.batch_size
        Xd, vols, idx = self._volumes(starts, goals, trajectories, prefer is None)
        if prefer is None:
            return idx, ctx.to_host(vols).reshape(S, B), None
        return self._pick(Xd, vols, (S, B), prefer, volume_trust_region)

    def choose_best_trajectories(self, starts, goals, trajectories, *, prefer=None, volume_trust_region: float = 0.0008):
        """choose_best_trajectory (lib/guide.py:637-653) for every scene: (S, 7, N), in the kind of array `trajectories` is"""
        idx, _, _ = self.select_rows(starts, goals, trajectories, prefer=prefer, volume_trust_region=volume_trust_region)
        S, B = self.n_scenes, self.batch_size
        rows = np.arange(S) * B + idx
        flat = trajectories.reshape(S * B, 7, -1)
        return flat[torch.as_tensor(rows, device=flat.device)] if isinstance(flat, torch.Tensor) else np.asarray(flat)[rows]

    def success_rows(self, trajectories, substeps: int = 4, return_device: bool = False):
        """IntersectionVolumeGuide.success_rows for every scene (edmp_scenes_success_rows_dev): the same dict, the per-row arrays ok,
        first, within, collision_free shaped (S, B) - each row checked against its own scene's obstacles and kinds - and the counts
        rows_ok, rows_within, rows_collision_free, rows as (S,) int arrays, one entry per scene."""
        Xd, N = self._state(trajectories)
        self._bind()
        return self._success(Xd, (self.n_scenes, self.batch_size), N, substeps, return_device)

    def self_collision_rows(self, trajectories, substeps: int = 4, pairs=None, return_device: bool = False):
        """IntersectionVolumeGuide.self_collision_rows for the (S, B, 7, N) / (S*B, 7, N) state in one call: first and free shaped
        (S, B), pair (S, B, 2).  The check reads nothing of the scenes: a row's answer is what any guide of this robot gives for it."""
        mask = franka.check_pair_mask(pairs)
        Xd, N = self._state(trajectories)
        self._bind()
        out = self._self_collision(Xd, (self.n_scenes, self.batch_size), N, substeps, mask, return_device)
        Xd.record_stream(self.ctx.stream)
        return out

    def sdf_rows(self, trajectories, starts, goals, t=0):
        """IntersectionVolumeGuide.sdf_rows for every scene (edmp_scenes_sdf_rows_dev): cost and minimum clearance of EVERY row of the
        (S, B, 7, N) / (S*B, 7, N) state under the sphere signed-distance model, each row against its own scene's primitives, kinds and
        start / goal pair -> {"cost": (S, B) f64, "clearance": (S, B) f64}; scene s's values are what guides[s].sdf_rows gives for
        X[s][:, :, 1:-1].  t = 0: margin 0; t >= 1: the rows' own margins at step t.  A batch built without SDF rows uses scene 0's
        sphere model (its ``spheres``, else the default of the link boxes) with margin 0 and smoothness 0 where the members bring none."""
        pair = _pairs(self.n_scenes, starts, goals)
        Xd, N = self._state(trajectories)
        self._bind_sdf()
        out = self._sdf_report(Xd, (self.n_scenes, self.batch_size), N, t, pair)
        Xd.record_stream(self.ctx.stream)
        return out

    def sdf_sweep_rows(self, trajectories, starts, goals, t=0, substeps=None):
        """IntersectionVolumeGuide.sdf_sweep_rows for every scene in one launch (edmp_scenes_sdf_sweep_rows_dev): the swept-clearance
        term's cost and the minimum clearance over the interpolants of EVERY row of the (S, B, 7, N) / (S*B, 7, N) state, each row
        against its own scene's primitives, kinds and start / goal pair -> {"cost": (S, B) f64, "clearance": (S, B) f64}; scene s's
        values are what guides[s].sdf_sweep_rows gives for X[s][:, :, 1:-1].  substeps=None: the rows' own weights and substeps;
        substeps=K: weight 1 and K on every row, t = 0 only.  Leaves a segmented run running."""
        pair = _pairs(self.n_scenes, starts, goals)
        Xd, N = self._state(trajectories)
        if substeps is None:
            self._bind_term("sweep")
        else:
            self._bind_sdf()
        out = self._sweep_report(Xd, (self.n_scenes, self.batch_size), N, t, pair, substeps)
        Xd.record_stream(self.ctx.stream)
        return out

    def repair_rows(self, trajectories, starts, goals, iters=32, substeps=4, margin=0.02, smoothness=0.5, step=0.02, max_step=0.02, rows=None,
                    return_device=False):
        """IntersectionVolumeGuide.repair_rows for every scene in one launch (edmp_scenes_sdf_repair_rows_dev): the (S, B, 7, N) /
        (S*B, 7, N) state, each row against its own scene's primitives, kinds and start / goal pair -> the same dict with trajectories
        (S, B, 7, N) and (S, B) per-row arrays; scene s's values are what guides[s].repair_rows gives for X[s].  ``rows`` indexes the S*B
        rows scene after scene.  Out of place; leaves a segmented run running."""
        pair = _pairs(self.n_scenes, starts, goals)
        Xd, N = self._state(trajectories)
        self._bind_sdf()
        out = self._repair(trajectories, Xd, (self.n_scenes, self.batch_size), N, pair, iters, substeps, margin, smoothness, step, max_step, rows, return_device)
        Xd.record_stream(self.ctx.stream)
        return out

    def shortcut_rows(self, trajectories, passes=2, substeps=4, min_gain=1e-6, rows=None, log_cap=128, return_device=False, self_pairs=None):
        """IntersectionVolumeGuide.shortcut_rows for every scene in one launch (edmp_scenes_shortcut_rows_dev): the (S, B, 7, N) /
        (S*B, 7, N) state, each row against its own scene's obstacles and kinds -> the same dict with trajectories (S, B, 7, N), (S, B)
        per-row arrays and spans (S, B, log_cap, 2); scene s's values are what guides[s].shortcut_rows gives for X[s].  ``rows`` indexes the
        S*B rows scene after scene.  0 <= ``passes`` <= 1024 (EDMP_MAX_SHORTCUT_PASSES).  ``self_pairs`` as there, ONE mask for all scenes
        (edmp_scenes_shortcut_rows_self_dev): self_rejected (S, B).  Out of place; leaves a segmented run running."""
        Xd, N = self._state(trajectories)
        self._bind()
        out = self._shortcut(trajectories, Xd, (self.n_scenes, self.batch_size), N, passes, substeps, min_gain, rows, log_cap, return_device, self_pairs)
        Xd.record_stream(self.ctx.stream)
        return out

    def certify_rows(self, trajectories, depth=6, margin=0.0, rows=None):
        """IntersectionVolumeGuide.certify_rows for every scene in one launch (edmp_scenes_certify_rows_dev): the (S, B, 7, N) /
        (S*B, 7, N) state as a HOST array (a device tensor is refused, as there), each row against its own scene's obstacles and kinds
        -> the same dict of host arrays with (S, B) per-row arrays; scene s's values are what guides[s].certify_rows gives for X[s].
        ``rows`` indexes the S*B rows scene after scene.  Read only; leaves a segmented run running."""
        Xd, N = self._state(self._host_state(trajectories))
        self._bind()
        out = self._certify(Xd, (self.n_scenes, self.batch_size), N, depth, margin, rows)
        Xd.record_stream(self.ctx.stream)
        return out

    def _flat_profile(self, profile, keys):
        """a profile dict shaped (S, B, ...) -> the arrays of `keys` it holds, shaped (S*B, ...)"""
        return {k: profile[k].reshape(self.n_scenes * self.batch_size, *profile[k].shape[2:]) for k in keys if k in profile}

    def _scene_profile(self, out, keys):
        """a profile dict shaped (S*B, ...) -> the same dict with the arrays of `keys` shaped (S, B, ...)"""
        for k in keys:
            out[k] = out[k].reshape(self.n_scenes, self.batch_size, *out[k].shape[1:])
        return out

    def time_rows(self, trajectories, vmax=None, amax=None, jump=None, scale=(1, 1), return_device: bool = False):
        """IntersectionVolumeGuide.time_rows for the (S, B, 7, N) / (S*B, 7, N) state in ONE launch (a reshape: the rule reads nothing of a
        scene) -> the profile dict with every array shaped (S, B, ...); scene s's values are bit for bit what guides[s].time_rows gives for
        X[s].  Leaves a segmented run running."""
        from .evaluation import PROFILE_KEYS, time_rows_on

        Xd, N = self._state(trajectories)
        return self._scene_profile(time_rows_on(self.ctx, Xd, vmax, amax, jump, scale, return_device), PROFILE_KEYS)

    def sample_rows(self, trajectories, profile, period, rows=None, max_samples=None, return_device: bool = False):
        """IntersectionVolumeGuide.sample_rows for the (S, B, 7, N) / (S*B, 7, N) state and the profile SceneBatch.time_rows gave, in ONE
        launch: ``rows`` indexes the S*B rows scene after scene (default all); q, qd (R, 7, M) and count (R,) in list order.  Leaves a
        segmented run running."""
        from .evaluation import PROFILE_KEYS, sample_rows_on

        Xd, N = self._state(trajectories)
        return sample_rows_on(self.ctx, Xd, self._flat_profile(profile, PROFILE_KEYS), period, rows, max_samples, return_device)

    def blend_rows(self, trajectories, deviation=0.01, reach=0.4, substeps=4, halvings=2, vmax=None, amax=None, jump=None, scale=(1, 1), rows=None,
                   return_device: bool = False, self_pairs=None):
        """IntersectionVolumeGuide.blend_rows for every scene in one launch (edmp_scenes_blend_rows_dev): the (S, B, 7, N) / (S*B, 7, N)
        state, each row against its own scene's obstacles and kinds -> the same dict with beta, code, halved (S, B, N) and tested (S, B);
        scene s's values are bit for bit what guides[s].blend_rows gives for X[s].  ``rows`` indexes the S*B rows scene after scene.
        ``self_pairs`` as there, ONE mask for all scenes (edmp_scenes_blend_rows_self_dev): self_hits (S, B, N).  Leaves a segmented run
        running."""
        Xd, N = self._state(trajectories)
        self._bind()
        out = self._blend(Xd, (self.n_scenes, self.batch_size), N, deviation, reach, substeps, halvings, vmax, amax, jump, scale, rows, return_device, self_pairs)
        Xd.record_stream(self.ctx.stream)
        return out

    def time_blended_rows(self, trajectories, beta, vmax=None, amax=None, jump=None, scale=(1, 1), return_device: bool = False):
        """IntersectionVolumeGuide.time_blended_rows for the (S, B, 7, N) / (S*B, 7, N) state and beta (S, B, N) / (S*B, N) in ONE launch ->
        the blended profile dict with every array shaped (S, B, ...); scene s's values are bit for bit what guides[s].time_blended_rows gives
        for X[s] and beta[s].  Leaves a segmented run running."""
        from .evaluation import BLENDED_PROFILE_KEYS, time_blended_rows_on

        Xd, N = self._state(trajectories)
        out = time_blended_rows_on(self.ctx, Xd, beta.reshape(self.n_scenes * self.batch_size, N), vmax, amax, jump, scale, return_device)
        return self._scene_profile(out, BLENDED_PROFILE_KEYS + ("beta",))

    def sample_blended_rows(self, trajectories, profile, period, rows=None, max_samples=None, return_device: bool = False):
        """IntersectionVolumeGuide.sample_blended_rows for the (S, B, 7, N) / (S*B, 7, N) state and the profile SceneBatch.time_blended_rows
        gave, in ONE launch: ``rows`` indexes the S*B rows scene after scene (default all); q, qd (R, 7, M) and count (R,) in list order.
        Leaves a segmented run running."""
        from .evaluation import BLENDED_PROFILE_KEYS, sample_blended_rows_on

        Xd, N = self._state(trajectories)
        return sample_blended_rows_on(self.ctx, Xd, self._flat_profile(profile, BLENDED_PROFILE_KEYS + ("beta",)), period, rows, max_samples, return_device)

    def sdf_self_rows(self, trajectories, t=0):
        """IntersectionVolumeGuide.sdf_self_rows for the (S, B, 7, N) / (S*B, 7, N) state (its interior columns 1..N-2 are the
        waypoints) in one call -> {"cost": (S, B) f64, "clearance": (S, B) f64}.  The term reads nothing of the scenes: scene s's values
        are what guides[s].sdf_self_rows gives for X[s][:, :, 1:-1]."""
        Xd, N = self._state(trajectories)
        self._bind_term("self")
        out = self._self_report(Xd, (self.n_scenes, self.batch_size), N, 1, N - 2, t)
        Xd.record_stream(self.ctx.stream)
        return out

    def sdf_goal_rows(self, trajectories, t=0, final=False):
        """IntersectionVolumeGuide.sdf_goal_rows for the (S, B, 7, N) / (S*B, 7, N) state (its interior columns 1..N-2 are the
        waypoints) in one call -> {"cost", "distance", "angle", "min_distance"}, each (S, B) f64, every row against its own scene's
        target: scene s's values are what guides[s].sdf_goal_rows gives for X[s][:, :, 1:-1].  final=True hands the goal column over as
        well (columns 1..N-1, as X[s][:, :, 1:]): distance and angle are then those of the plan's final tool pose."""
        Xd, N = self._state(trajectories)
        self._bind_term("goal")
        out = self._goal_report(Xd, (self.n_scenes, self.batch_size), N, 1, N - 1 if final else N - 2, t)
        Xd.record_stream(self.ctx.stream)
        return out
