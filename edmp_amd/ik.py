"""IK goal candidates of the 7-DoF Franka on the GPU: damped least squares from many seeds (edmp_ik_solve_dev / edmp_ik_compact_dev,
csrc/ik.hip), every seed of every target of a scene group in one launch.

Stands for the reference's `FrankaRobot.ik(target)` (datasets/load_test_dataset.py:170-187: robofin's analytic ikfast, 100 candidates
per scene), which this package neither ships nor restates: the candidates here are other points of the same solution continuum, each
reproducing the target pose to `tol_pos` / `tol_ang`.  What happens to them afterwards - the IK-goal filter - is unchanged.

    ik = FrankaIK("cuda:0", n_seeds=256, seed=0, tool=my_gripper_frame)
    dataset = ProblemSetDataset(path, ik=ik)                  # (xyz, quaternion_wxyz) -> (n, 7)
    res = solve("cuda:0", targets, 256, return_device=True)   # a group: dense device goals + counts -> SceneBatch.filter_goals

Frames.  The pose that is matched is (joint-7 frame of the modified-DH chain, lib/guide.py:29-35) x (tool frame).  `tool=None` is the
reference's own end-effector chain (rows 8-10 of its table = evaluation.EE_STATIC_DH, lib/guide.py:100-116); "flange" and "hand" are the
two frames the reference's URDF defines behind joint 7 (d = 0.107; then rpy = (0, 0, -pi/4)); a (4, 4) / (3, 4) array is taken as given.
There is no `right_gripper` preset: MPiNets targets are in that frame, and its offset from the flange is defined by robofin's URDF, which
this package cannot cite - the caller passes it as `tool=`.

Seeds come from a private RandomState: the global NumPy stream is the reference's noise contract and the driver's feeder thread is
advancing it while scenes are prepared.  Runs on the GPU only: there is no host solver."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import evaluation, franka

ITERS, DAMPING, MAX_STEP, TOL_POS, TOL_ANG = 64, 0.01, 0.5, 1e-6, 1e-6
ORTHONORMAL_TOL = 1e-9  # the C-ABI's own bound on |R^T R - I|
TOOL_NAMES = ("flange", "hand")


def draw_seeds(n, seed, start=None) -> np.ndarray:
    """(n, 7) f64 uniform inside franka.joint_limits(), from a private np.random.RandomState(seed) - never the global stream.  With
    `start` (7,), row 0 is `start` clipped to the limits (a candidate near the start configuration) and the draws fill the rest."""
    n = int(n)
    if n < 1:
        raise ValueError(f"need n >= 1 seeds, got {n}")
    lo, hi = franka.joint_limits()
    q = np.random.RandomState(int(seed)).uniform(lo, hi, (n, 7))
    q = np.minimum(np.maximum(q, lo), hi)  # (lo + (hi - lo) * u can round one ulp past hi)
    if start is not None:
        s = np.asarray(start, dtype=np.float64)
        if s.shape != (7,) or not np.isfinite(s).all():
            raise ValueError(f"start must be 7 finite joint angles, got shape {s.shape}")
        q[0] = np.clip(s, lo, hi)
    return q


def _check_frame(m, what) -> np.ndarray:
    """(4, 4) or (3, 4) -> (3, 4) f64 [R | p], finite, R orthonormal to ORTHONORMAL_TOL and no reflection"""
    a = np.asarray(m, dtype=np.float64)
    if a.shape == (4, 4):
        if not np.array_equal(a[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError(f"{what}: the last row of a (4, 4) frame must be [0, 0, 0, 1]")
        a = a[:3]
    if a.shape != (3, 4):
        raise ValueError(f"{what} must be (4, 4) or (3, 4), got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} holds non-finite values")
    R = a[:, :3]
    dev = float(np.max(np.abs(R.T @ R - np.eye(3))))
    if dev > ORTHONORMAL_TOL or np.linalg.det(R) <= 0:
        raise ValueError(f"{what}: the rotation is not orthonormal to {ORTHONORMAL_TOL:g} (|R^T R - I| = {dev:.3g}) or is a reflection")
    return np.ascontiguousarray(a)


def tool_frame(tool=None) -> np.ndarray:
    """the (3, 4) f64 tool frame behind the joint-7 frame: None | "flange" | "hand" | a (4, 4) / (3, 4) array (module docstring)"""
    if tool is None:
        rows = evaluation.EE_STATIC_DH
    elif isinstance(tool, str):
        if tool not in TOOL_NAMES:
            raise ValueError(f"unknown tool {tool!r}: None (the reference's end-effector chain), {', '.join(repr(t) for t in TOOL_NAMES)} or a (4, 4) frame "
                             "(there is no 'right_gripper' preset: pass that frame's offset from the joint-7 frame as an array)")
        rows = evaluation.EE_STATIC_DH[:1] if tool == "flange" else evaluation.EE_STATIC_DH[:2]
    else:
        return _check_frame(tool, "tool")
    T = np.eye(4)
    for a, d, al, th in rows:
        T = T @ evaluation._dh(a, d, al, th)
    return np.ascontiguousarray(T[:3])


def pose_matrix(xyz, quaternion_wxyz) -> np.ndarray:
    """(3, 4) f64 [R | p] of a position and a scalar-first quaternion (normalised here)"""
    p = np.asarray(xyz, dtype=np.float64)
    qt = np.asarray(quaternion_wxyz, dtype=np.float64)
    if p.shape != (3,) or qt.shape != (4,):
        raise ValueError(f"a target pair is (xyz (3,), quaternion_wxyz (4,)), got {p.shape}, {qt.shape}")
    n = float(np.linalg.norm(qt))
    if not (np.isfinite(p).all() and np.isfinite(n) and n > 0):
        raise ValueError("target holds non-finite values or a zero quaternion")
    w, x, y, z = qt / n
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([R, p[:, None]], axis=1)


def target_matrices(targets) -> np.ndarray:
    """(T, 4, 4) / (T, 3, 4) array, or a list of (xyz, quaternion_wxyz) pairs or of such matrices -> checked (T, 3, 4) f64"""
    if isinstance(targets, np.ndarray) and targets.dtype != object:
        if targets.ndim != 3:
            raise ValueError(f"targets must be (T, 4, 4) or (T, 3, 4), got {targets.shape}")
        items = list(targets)
    else:
        items = list(targets)
    if not items:
        raise ValueError("no targets")
    out = []
    for t, it in enumerate(items):
        if isinstance(it, (tuple, list)) and len(it) == 2 and np.ndim(it[0]) == 1:
            it = pose_matrix(it[0], it[1])
        out.append(_check_frame(it, f"target {t}"))
    return np.ascontiguousarray(np.stack(out))


def check_params(iters, damping, max_step, tol_pos, tol_ang):
    if int(iters) != iters or int(iters) < 1:
        raise ValueError(f"iters must be an integer >= 1, got {iters!r}")
    vals = dict(damping=damping, max_step=max_step, tol_pos=tol_pos, tol_ang=tol_ang)
    for k, v in vals.items():
        if not np.isfinite(float(v)):
            raise ValueError(f"{k} must be finite, got {v!r}")
    if not float(damping) > 0:
        raise ValueError(f"damping (lambda) must be > 0, got {damping!r}: J J^T + lambda^2 I must be positive definite")
    if not float(max_step) > 0:
        raise ValueError(f"max_step must be > 0, got {max_step!r}")
    if float(tol_pos) < 0 or float(tol_ang) < 0:
        raise ValueError(f"tol_pos and tol_ang must be >= 0, got {tol_pos!r}, {tol_ang!r}")
    return int(iters), float(damping), float(max_step), float(tol_pos), float(tol_ang)


def seed_arrays(n_targets, seeds, seed=0):
    """`seeds` of solve(): an int n (the same draw_seeds(n, seed) for every target, so that a target's candidates do not depend on the
    group it is solved in) or a list of T arrays (n_t, 7), n_t >= 1, finite and inside the joint limits -> (flat (sum, 7) f64, counts (T,) int32)"""
    T = int(n_targets)
    if isinstance(seeds, (int, np.integer)) and not isinstance(seeds, bool):
        one = draw_seeds(seeds, seed)
        return np.ascontiguousarray(np.concatenate([one] * T)), np.full(T, one.shape[0], dtype=np.int32)
    if isinstance(seeds, np.ndarray) and seeds.dtype != object:
        seeds = list(seeds) if seeds.ndim == 3 else None
    if seeds is None or isinstance(seeds, (str, bytes, float)) or len(seeds) != T:
        raise ValueError(f"seeds must be an int or a list of {T} arrays (n_t, 7), one per target")
    lo, hi = franka.joint_limits()
    out = []
    for t, s in enumerate(seeds):
        a = np.asarray(s, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 7 or a.shape[0] < 1:
            raise ValueError(f"seeds[{t}] must be (n, 7) with n >= 1, got {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"seeds[{t}] holds non-finite values")
        if (a < lo).any() or (a > hi).any():
            raise ValueError(f"seeds[{t}] leaves the joint limits (franka.joint_limits(); draw_seeds stays inside)")
        out.append(a)
    return np.ascontiguousarray(np.concatenate(out)), np.asarray([a.shape[0] for a in out], dtype=np.int32)


def solve(ctx_or_device, targets, seeds=256, *, seed=0, tool=None, iters=ITERS, damping=DAMPING, max_step=MAX_STEP, tol_pos=TOL_POS, tol_ang=TOL_ANG,
          return_device=False, return_all=False) -> dict:
    """Solve every target from every one of its seeds in one launch, keep the valid solutions.

    targets: (T, 4, 4) / (T, 3, 4) poses of the tool frame in the base frame, or a list of (xyz, quaternion_wxyz) pairs.  seeds: an int
    (that many draw_seeds(n, seed) rows, the same for every target) or a list of T arrays (n_t, 7).  tool: see tool_frame.
    Returns dict(counts (T,) int32, goals): goals is a list of T arrays (count_t, 7) f64 - each target's valid solutions in seed order,
    possibly empty - or, with return_device, the dense (sum counts, 7) f64 device tensor, target after target: with `counts` the device
    form SceneBatch.filter_goals takes.  return_all adds the per-seed q (sum, 7), residuals (sum, 2) [position m, angle rad], valid (sum,)
    bool and n_seeds (T,) (device tensors with return_device, valid then int32).  Wrong shapes, non-finite values, seeds outside the limits, a
    rotation that is not orthonormal and bad parameters raise ValueError before the GPU is touched."""
    tg = target_matrices(targets)
    tl = tool_frame(tool)
    iters, damping, max_step, tol_pos, tol_ang = check_params(iters, damping, max_step, tol_pos, tol_ang)
    flat, counts_in = seed_arrays(tg.shape[0], seeds, seed)

    import torch

    from . import _capi
    from .runtime import get_context, ptr

    ctx = get_context(ctx_or_device)
    T, n = int(tg.shape[0]), int(flat.shape[0])
    sd = ctx.to_dev(flat, torch.float64)
    q = ctx.empty((n, 7), torch.float64)
    res = ctx.empty((n, 2), torch.float64)
    valid = ctx.empty((n,), torch.int32)
    goals = ctx.empty((n, 7), torch.float64)
    tg12 = np.ascontiguousarray(tg.reshape(T, 12))
    tl12 = np.ascontiguousarray(tl.reshape(12))
    _capi.check(ctx.lib.edmp_ik_solve_dev(ctx.h, _capi.as_pd(tg12), T, _capi.as_pi32(counts_in), ptr(sd), _capi.as_pd(tl12), iters, C.c_double(damping),
                                          C.c_double(max_step), C.c_double(tol_pos), C.c_double(tol_ang), ptr(q), ptr(res), ptr(valid)), "edmp_ik_solve_dev")
    counts = np.zeros(T, dtype=np.int32)
    _capi.check(ctx.lib.edmp_ik_compact_dev(ctx.h, ptr(q), ptr(valid), T, _capi.as_pi32(counts_in), ptr(goals), _capi.as_pi32(counts)), "edmp_ik_compact_dev")
    total = int(counts.sum())
    out = dict(counts=counts)
    if return_device:
        for t in (goals, q, res, valid):
            ctx.hand_over(t)
        out["goals"] = goals[:total]
        if return_all:
            out.update(q=q, residuals=res, valid=valid, n_seeds=counts_in)
        return out
    gh = ctx.to_host(goals[:total]) if total else np.zeros((0, 7))
    off = np.concatenate([[0], np.cumsum(counts)])
    out["goals"] = [gh[off[t]:off[t + 1]].copy() for t in range(T)]
    if return_all:
        out.update(q=ctx.to_host(q), residuals=ctx.to_host(res), valid=ctx.to_host(valid).astype(bool), n_seeds=counts_in)
    return out


class FrankaIK:
    """The `ik=` callable of scenes.ProblemSetDataset: (xyz, quaternion_wxyz) -> (n, 7) valid goal candidates in seed order, n <= n_seeds,
    from draw_seeds(n_seeds, seed) (the same seeds for every target: a target's candidates do not depend on when or with what it is
    solved).  ValueError naming the target when no seed converged.  solve_many does a group of targets in one launch."""

    def __init__(self, device="cuda:0", n_seeds=256, seed=0, tool=None, iters=ITERS, damping=DAMPING, max_step=MAX_STEP, tol_pos=TOL_POS, tol_ang=TOL_ANG):
        self.device, self.n_seeds, self.seed = device, int(n_seeds), int(seed)
        if self.n_seeds < 1:
            raise ValueError(f"n_seeds must be >= 1, got {n_seeds}")
        self.tool = tool_frame(tool)
        self.params = dict(zip(("iters", "damping", "max_step", "tol_pos", "tol_ang"), check_params(iters, damping, max_step, tol_pos, tol_ang)))

    def solve_many(self, targets, return_device=False) -> dict:
        """solve() for a group of targets with this object's seeds, tool and parameters; ValueError naming the first target without a
        valid solution"""
        tg = target_matrices(targets)
        r = solve(self.device, tg, self.n_seeds, seed=self.seed, tool=self.tool, return_device=return_device, **self.params)
        for t, c in enumerate(r["counts"]):
            if c < 1:
                raise ValueError(f"IK: none of {self.n_seeds} seeds converged for target {t} (position {tg[t][:, 3].tolist()}): unreachable within "
                                 f"{self.params['tol_pos']:g} m / {self.params['tol_ang']:g} rad in {self.params['iters']} iterations, or the wrong tool frame")
        return r

    def __call__(self, xyz, quaternion_wxyz) -> np.ndarray:
        return self.solve_many([(xyz, quaternion_wxyz)])["goals"][0]
