"""Result evaluation: plan success over the whole batch (on the GPU) and trajectory metrics (host like the reference's, and whole batches on the GPU).

Success.  The reference scores a plan by executing it in pybullet (`RobotEnvironment.benchmark_trajectory`,
lib/environment.py:632-680: position control through the waypoints, contact query `check_collisions` :591-608 against
spawned cuboids AND true cylinders :230-268) and tallies `t_success` (infer_serial.py:94-99,165-168).  pybullet is not
available offline, so the criterion is restated geometrically — EXACT oriented-box / finite-cylinder tests instead of the
guide's conservative world-AABB overlap — and evaluated for every row of the batch by `edmp_success_rows_dev`
(csrc/success.hip) through `IntersectionVolumeGuide.success_rows`, and for the S * B rows of a scene batch, each against its own scene, by
`edmp_scenes_success_rows_dev` through `SceneBatch.success_rows`.  It is a stand-in (no dynamics, box-shaped links),
reported as such.  There is no host fallback: the checker of the kernel lives in oracle/success_oracle.py (tests only).

Metrics.  lib/metrics.py:11-125 (`MetricsCalculator`, host NumPy / torch-CPU in the reference too, never called by its
driver): path length and SPARC smoothness, pinned to the reference by tests/golden/g13_metrics.npz.  `path_lengths`, `sparc`,
`smoothness_metric` score ONE trajectory on the host; `batch_metrics` scores every row of a batch on the GPU (edmp_metrics_rows_dev,
csrc/metrics.hip) and is checked against them; `ensemble_report` turns volumes, success flags and metrics into the per-guide table.
"""
from __future__ import annotations

import numpy as np

from . import franka


def _dh(a, d, alpha, q):
    cq, sq, ca, sa = np.cos(q), np.sin(q), np.cos(alpha), np.sin(alpha)
    return np.array([[cq, -sq, 0, a], [sq * ca, cq * ca, -sa, -sa * d], [sq * sa, cq * sa, ca, ca * d], [0, 0, 0, 1.0]])


def geometric_success(trajectory, guide, substeps: int = 4) -> dict:
    """ONE trajectory (7, N) against the scene of `guide` (an IntersectionVolumeGuide): dict(success, collision_free,
    first_collision_waypoint, within_limits).  `collision_free` is the reference's success flag (lib/environment.py:672: contact
    only; leaving the limits merely prints, :659-661), `success` additionally requires `within_limits`.  Runs on the GPU (one-row
    batch of guide.success_rows)."""
    tr = np.asarray(trajectory, dtype=np.float64)
    if tr.ndim != 2 or tr.shape[0] != 7:
        raise ValueError(f"trajectory must be (7, N), got {tr.shape}")
    r = guide.success_rows(tr[None], substeps=substeps)
    return dict(success=bool(r["ok"][0]), collision_free=bool(r["collision_free"][0]), first_collision_waypoint=int(r["first"][0]), within_limits=bool(r["within"][0]))


def success_rate(trajectories, guide, substeps: int = 4) -> dict:
    """every row of a batch (B, 7, N): dict(rows_ok, rows, rate, ok (B,), first (B,), within (B,)) - the batch form of the
    reference's running tally `t_success / i` (infer_serial.py:99).  `guide` may be a guide.SceneBatch with trajectories (S, B, 7, N) or
    (S*B, 7, N): the per-row arrays are then (S, B) and the counts and rates (S,), one entry per scene (one launch for all scenes)."""
    r = guide.success_rows(trajectories, substeps=substeps)
    rows = np.maximum(r["rows"], 1) if np.ndim(r["rows"]) else max(r["rows"], 1)
    r["rate"] = r["rows_ok"] / rows
    r["collision_free_rate"] = r["rows_collision_free"] / rows  # the reference's criterion (lib/environment.py:672)
    return r


def self_collision_rate(trajectories, guide, substeps: int = 4, pairs=None) -> dict:
    """every row of a batch (n, 7, N) checked for self-collision on the GPU (guide.self_collision_rows, csrc/selfcol.hip; stands for the
    `self_collision` metric of the reference's evaluation package, mpinets/metrics.py:278-292): that dict (first, pair, free) plus
    rows_free, rows and rate = the share of self-collision-free rows.  `guide` may be a guide.SceneBatch with trajectories (S, B, 7, N) or
    (S*B, 7, N): the per-row arrays are then (S, B), the counts and rates (S,).  ``pairs``: the (9, 9) mask of checked link pairs,
    default franka.self_collision_pairs()."""
    r = guide.self_collision_rows(trajectories, substeps=substeps, pairs=pairs)
    free = np.asarray(r["free"])
    per_scene = free.ndim == 2
    r["rows_free"] = free.sum(axis=-1).astype(np.int64) if per_scene else int(free.sum())
    r["rows"] = np.full(free.shape[0], free.shape[1], dtype=np.int64) if per_scene else int(free.shape[0])
    r["rate"] = r["rows_free"] / np.maximum(r["rows"], 1)
    return r


# the fixed flange / hand chain behind joint 7: rows 8-10 of the reference's modified-DH table [a, d, alpha, theta]
# (lib/guide.py:36-38), used only by get_end_effector_transform (lib/guide.py:100-116)
EE_STATIC_DH = ((0.0, 0.107, 0.0, 0.0), (0.0, 0.0, 0.0, -np.pi / 4), (0.0, 0.1034, 0.0, 0.0))


def end_effector_positions(trajectory):
    """(N, 3) end-effector positions as lib/metrics.py computes them: the translation of
    IntersectionVolumeGuide.get_end_effector_transform (lib/guide.py:100-116), i.e. ALL TEN modified-DH rows - the seven
    joints followed by the fixed rows d = 0.107, theta = -pi/4, d = 0.1034 (0.21 m beyond the joint-7 frame).
    float64 here, float32 in the reference: agrees to ~1e-7 m (pinned by tests/golden/g13_metrics.npz)."""
    tr = np.asarray(trajectory, dtype=np.float64)
    n = tr.shape[1]

    def dh_stack(a, d, alpha, q):  # (N, 4, 4): _dh for every waypoint at once (a per-waypoint Python loop cost 2 ms per call)
        cq, sq, ca, sa = np.cos(q), np.sin(q), np.cos(alpha), np.sin(alpha)
        D = np.zeros((n, 4, 4))
        D[:, 0, 0], D[:, 0, 1], D[:, 0, 3] = cq, -sq, a
        D[:, 1, 0], D[:, 1, 1], D[:, 1, 2], D[:, 1, 3] = sq * ca, cq * ca, -sa, -sa * d
        D[:, 2, 0], D[:, 2, 1], D[:, 2, 2], D[:, 2, 3] = sq * sa, cq * sa, ca, ca * d
        D[:, 3, 3] = 1.0
        return D

    T = np.broadcast_to(np.eye(4), (n, 4, 4))
    for j in range(7):
        a, d, al = franka.DH_A_D_ALPHA[j]
        T = T @ dh_stack(a, d, al, tr[j])
    for a, d, al, th in EE_STATIC_DH:
        T = T @ _dh(a, d, al, th)
    return np.ascontiguousarray(T[:, :3, 3])


def tool_pose_errors(q, target, tool=None) -> dict:
    """ONE configuration q (7,) against a target pose, on the host in float64: the pose (joint-7 frame of the modified-DH chain) x
    (tool frame, whatever ik.tool_frame takes) compared with `target` ((xyz, quaternion_wxyz) or a (4, 4) / (3, 4) pose) ->
    dict(distance [m], angle [rad] = atan2(||a|| / 2, (tr - 1) / 2) with a = sum_k c*_k x c_k: exact near 0 and near pi,
    position_error [cm] and orientation_error [deg], the units of the reference's evaluator (mpinets/metrics.py:364-385), and
    e_pos = distance^2, e_ori = 3 - tr(R*^T R) = 4 sin^2(angle / 2), the two parts of the SDF guide's goal term, csrc/sdf.hip).
    The checker of edmp_sdf_goal_rows_dev and the unit test of the driver's report."""
    from . import ik

    qv = np.asarray(q, dtype=np.float64)
    if qv.shape != (7,):
        raise ValueError(f"q must be 7 joint angles, got shape {qv.shape}")
    tg = ik.pose_matrix(*target) if isinstance(target, (tuple, list)) and len(target) == 2 and np.ndim(target[0]) == 1 else target
    tg = ik._check_frame(tg, "target")
    T = np.eye(4)
    for j in range(7):
        a, d, al = franka.DH_A_D_ALPHA[j]
        T = T @ _dh(a, d, al, qv[j])
    P = T[:3] @ np.vstack([ik.tool_frame(tool), [0.0, 0.0, 0.0, 1.0]])
    R, Rt = P[:, :3], tg[:, :3]
    dp = P[:, 3] - tg[:, 3]
    av = np.sum(np.cross(Rt.T, R.T), axis=0)  # sum over the columns k of c*_k x c_k
    tr = float(np.sum(Rt * R))
    dist, ang = float(np.linalg.norm(dp)), float(np.arctan2(np.linalg.norm(av) / 2, (tr - 1) / 2))
    return dict(distance=dist, angle=ang, position_error=100.0 * dist, orientation_error=float(np.degrees(ang)), e_pos=float(dp @ dp), e_ori=3.0 - tr)


def path_lengths(trajectory) -> dict:
    """MetricsCalculator.path_length_metric (lib/metrics.py:32-45): joint-space and end-effector path length."""
    tr = np.asarray(trajectory, dtype=np.float64)
    ee = end_effector_positions(tr)
    return dict(joint=float(np.sum(np.linalg.norm(np.diff(tr.T, 1, axis=0), axis=1))), end_effector=float(np.sum(np.linalg.norm(np.diff(ee, 1, axis=0), axis=1))))


def sparc(speed_profile, fs: float, padlevel: int = 4, fc: float = 10.0, amp_th: float = 0.05) -> float:
    """Spectral arc length smoothness (Balasubramanian et al. 2015): the value `MetricsCalculator.sparc`
    (lib/metrics.py:47-125, a restatement of mpinets/third_party/sparc.py) returns first.  More negative = less smooth;
    an all-zero profile returns 0 like the reference."""
    v = np.asarray(speed_profile, dtype=np.float64)
    if np.allclose(v, 0):
        return 0.0
    nfft = int(pow(2, np.ceil(np.log2(len(v))) + padlevel))
    f = np.arange(0, fs, fs / nfft)
    Mf = np.abs(np.fft.fft(v, nfft))
    Mf = Mf / Mf.max()
    sel = np.nonzero(f <= fc)[0]
    f_sel, Mf_sel = f[sel], Mf[sel]
    idx = np.nonzero(Mf_sel >= amp_th)[0]
    f_sel, Mf_sel = f_sel[idx[0] : idx[-1] + 1], Mf_sel[idx[0] : idx[-1] + 1]
    return float(-np.sum(np.sqrt((np.diff(f_sel) / (f_sel[-1] - f_sel[0])) ** 2 + np.diff(Mf_sel) ** 2)))


def smoothness_metric(trajectory, dt: float = 0.1) -> tuple:
    """MetricsCalculator.smoothness_metric (lib/metrics.py:11-30): (joint SPARC, end-effector SPARC) of the speed
    profiles ||diff / dt|| of the (7, N) joint trajectory and of its end-effector positions."""
    tr = np.asarray(trajectory, dtype=np.float64)
    js = np.linalg.norm(np.diff(tr.T, n=1, axis=0) / dt, axis=1)
    ee = end_effector_positions(tr)
    es = np.linalg.norm(np.diff(ee, n=1, axis=0) / dt, axis=1)
    return sparc(js, 1.0 / dt), sparc(es, 1.0 / dt)


def smoothness(trajectory, dt: float = 0.1) -> float:
    """joint-space SPARC of a (7, N) trajectory (first component of smoothness_metric)."""
    return smoothness_metric(trajectory, dt)[0]


METRIC_KEYS = ("joint_path_length", "ee_path_length", "joint_sparc", "ee_sparc")  # row order of edmp_metrics_rows_dev's (4, B) output


def metrics_rows_on(ctx, trajectories, dt: float = 0.1, return_device: bool = False) -> dict:
    """edmp_metrics_rows_dev on the context `ctx` (runtime.Context): see batch_metrics."""
    import ctypes as C

    import torch

    from . import _capi
    from .runtime import ptr

    if isinstance(trajectories, torch.Tensor) and trajectories.is_cuda:
        X = ctx.adopt(trajectories.to(torch.float64).contiguous())
    else:
        X = ctx.to_dev(np.asarray(trajectories, dtype=np.float64), torch.float64)
    if X.dim() != 3 or X.shape[1] != 7:
        raise ValueError(f"trajectories must be (B, 7, N), got {tuple(X.shape)}")
    B, N = X.shape[0], X.shape[2]
    out = ctx.empty((4, B), torch.float64)
    dh = np.ascontiguousarray(franka.dh_table_f64())
    _capi.check(ctx.lib.edmp_metrics_rows_dev(ctx.h, ptr(X), B, N, C.c_double(float(dt)), _capi.as_pd(dh), ptr(out)), "edmp_metrics_rows_dev")
    if return_device:
        X.record_stream(ctx.stream)  # (the kernel may still be reading it when the caller drops the tensor)
        ctx.hand_over(out)
        return {k: out[i] for i, k in enumerate(METRIC_KEYS)}
    h = ctx.to_host(out)
    return {k: h[i].copy() for i, k in enumerate(METRIC_KEYS)}


def batch_metrics(trajectories, device="cuda:0", dt: float = 0.1, return_device: bool = False) -> dict:
    """The reference's result metrics (lib/metrics.py:11-125, MetricsCalculator) for EVERY row of a batch in one kernel
    (edmp_metrics_rows_dev, csrc/metrics.hip): trajectories (B, 7, N) ndarray or device tensor, 3 <= N <= 129 -> dict of four (B,)
    float64 arrays joint_path_length, ee_path_length, joint_sparc, ee_sparc (device tensors with return_device).  Row b equals
    path_lengths(trajectories[b]) and smoothness_metric(trajectories[b], dt) - the single-trajectory host functions above, which stay
    the yardstick - to 1e-9; a row whose speed profile is not finite gets SPARC = NaN where the host functions raise.  Needs no scene
    and no guide.  Runs on the GPU only: there is no host fallback."""
    from .runtime import get_context

    return metrics_rows_on(get_context(device), trajectories, dt, return_device)


PROFILE_KEYS = ("y", "phase", "times", "duration", "limit", "seg")  # edmp_time_rows_dev's outputs, what edmp_sample_rows_dev reads
BLENDED_PROFILE_KEYS = PROFILE_KEYS + ("blend",)  # edmp_time_blended_rows_dev's outputs; the profile dict also carries `beta`
LIMIT_NAMES = ("rest", "velocity_before", "velocity_after", "corner_jump", "acceleration", "deceleration")  # the codes of `limit`


def _rows_state(ctx, trajectories):
    """(n, 7, N) ndarray or device tensor -> the contiguous f64 device tensor on ctx's stream"""
    import torch

    if isinstance(trajectories, torch.Tensor) and trajectories.is_cuda:
        X = ctx.adopt(trajectories.to(torch.float64).contiguous())
    else:
        X = ctx.to_dev(np.asarray(trajectories, dtype=np.float64), torch.float64)
    if X.dim() != 3 or X.shape[1] != 7:
        raise ValueError(f"trajectories must be (n, 7, N), got {tuple(X.shape)}")
    return X


def _device_f64(ctx, v, want, name, X):
    """an array or device tensor that goes with the state X -> the contiguous f64 device tensor on ctx's stream, its shape checked"""
    import torch

    t = ctx.adopt(v.to(torch.float64).contiguous()) if isinstance(v, torch.Tensor) and v.is_cuda else ctx.to_dev(np.asarray(v, dtype=np.float64), torch.float64)
    if tuple(t.shape) != want:
        raise ValueError(f"{name} must be {want} for trajectories {tuple(X.shape)}, got {tuple(t.shape)}")
    return t


def _time_rows(ctx, X, beta, limits, return_device):
    """The one timing call behind time_rows_on (beta None: edmp_time_rows_dev, PROFILE_KEYS) and time_blended_rows_on (beta (n, N):
    edmp_time_blended_rows_dev, BLENDED_PROFILE_KEYS, two times per waypoint, beta in the result).  X and beta: device tensors that the
    caller has brought onto ctx's stream; limits = (vmax, amax, jump)."""
    import torch

    from . import _capi
    from .runtime import ptr

    blended = beta is not None
    entry, keys, given = ("edmp_time_blended_rows_dev", BLENDED_PROFILE_KEYS, (X, beta)) if blended else ("edmp_time_rows_dev", PROFILE_KEYS, (X,))
    n, N = X.shape[0], X.shape[2]
    shape = dict(y=(n, N), phase=(n, max(N - 1, 0), 3), times=(n, N, 2) if blended else (n, N), duration=(n,), limit=(n, N), seg=(n, max(N - 1, 0), 2),
                 blend=(n, N))
    out = {k: ctx.empty(shape[k], torch.int32 if k == "limit" else torch.float64) for k in keys}
    _capi.check(getattr(ctx.lib, entry)(ctx.h, ptr(X), n, N, *(ptr(t) for t in given[1:]), *(_capi.as_pd(v) for v in limits), *(ptr(out[k]) for k in keys)), entry)
    if return_device:
        for t in given:
            t.record_stream(ctx.stream)  # (the kernel may still be reading it when the caller drops the tensor)
        for k in keys:
            ctx.hand_over(out[k])
    else:
        out = {k: ctx.to_host(out[k]) for k in keys}
    if blended:
        out["beta"] = beta if return_device else ctx.to_host(beta)
    out.update(zip(("vmax", "amax", "jump"), limits))
    return out


def time_rows_on(ctx, trajectories, vmax=None, amax=None, jump=None, scale=(1, 1), return_device: bool = False) -> dict:
    """edmp_time_rows_dev on the context `ctx` (runtime.Context): see time_rows."""
    limits = franka.timing_limits(vmax, amax, jump, scale)
    return _time_rows(ctx, _rows_state(ctx, trajectories), None, limits, return_device)


def time_rows(trajectories, vmax=None, amax=None, jump=None, scale=(1, 1), device="cuda:0", return_device: bool = False) -> dict:
    """Time EVERY finished row under joint velocity, acceleration and corner velocity-jump limits (edmp_time_rows_dev, csrc/timing.hip; the
    reference replays its plans at constant velocity and ships no timing): trajectories (n, 7, N) ndarray or device tensor, 2 <= N <= 64 ->
    the profile of the fastest rest-to-rest motion ALONG each row's polyline: dict(y (n, N) = squared path speed at the waypoints, phase
    (n, N-1, 3) = accelerate | cruise | decelerate times of each segment [s], times (n, N) waypoint times, duration (n,) [s], limit (n, N)
    int32 = the constraint that binds each waypoint (index into LIMIT_NAMES), seg (n, N-1, 2) = path acceleration | peak squared speed of
    each segment; device tensors with return_device) plus the limits used, vmax / amax / jump (7,).  Limits: franka.timing_limits - Franka's
    published joint velocity and acceleration limits times scale = (sv, sa), and an illustrative corner jump of amax * 1 ms.  The rule is
    stated in include/edmp_hip.h.  |qdot| <= vmax everywhere, |qddot| <= amax inside segments, the velocity jump at a corner <= jump, and
    the path is the input polyline: what success_rows, self_collision_rows and shortcut_rows said of the row holds for the timed motion.  A
    row with a non-finite element is not timed (NaN, limit -1).  Needs no scene and no guide.  Runs on the GPU only."""
    from .runtime import get_context

    return time_rows_on(get_context(device), trajectories, vmax, amax, jump, scale, return_device)


def sample_count(duration, period) -> int:
    """1 + the smallest k with float(k) * period >= duration: the samples of a row up to and including the first one at rest at the goal
    (edmp_sample_rows_dev states its count the same way); 0 for a row that was not timed"""
    duration, period = float(duration), float(period)
    if not np.isfinite(duration):
        return 0
    k = int(np.ceil(duration / period))
    while k > 0 and float(k - 1) * period >= duration:
        k -= 1
    while float(k) * period < duration:
        k += 1
    return 1 + k


def _sample_setup(ctx, X, want, profile, period, rows, max_samples):
    """what both samplers settle before their call: the period, the checked row list, M, the output tensors and the arrays of `want`
    (name -> shape) that the entry reads of the profile, on ctx's stream -> (period, listed, R, M, q, qd, count, prof)"""
    import torch

    n = X.shape[0]
    period = float(period)
    if not (np.isfinite(period) and period > 0):
        raise ValueError(f"period must be finite and > 0, got {period!r}")
    listed = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
    if listed is not None and listed.size and (listed.min() < 0 or listed.max() >= n):
        raise ValueError(f"rows must lie in 0..{n - 1}, got {listed.tolist()}")
    dur = profile["duration"]
    if isinstance(dur, torch.Tensor):  # read on this context's stream, so adopted HERE: the trajectories may be a host array, and then nothing was adopted yet
        dur = ctx.to_host(ctx.adopt(dur) if dur.is_cuda else dur)
    dur = np.asarray(dur, dtype=np.float64).reshape(-1)
    order = np.arange(n) if listed is None else listed
    counts = [sample_count(dur[r], period) for r in order]
    if max_samples is None:
        M = max(1, max(counts, default=1))
    else:
        M = int(max_samples)
        short = [(int(r), c) for r, c in zip(order, counts) if c > M]
        if short:
            raise ValueError(f"max_samples = {M} is smaller than the {short[0][1]} samples of row {short[0][0]}")
    R = int(order.shape[0])
    with torch.cuda.stream(ctx.stream):
        q = torch.empty((R, 7, max(M, 0)), dtype=torch.float64, device=ctx.device)
        qd = torch.empty_like(q)
        count = torch.empty((R,), dtype=torch.int32, device=ctx.device)
    prof = {k: _device_f64(ctx, profile[k], want[k], f"profile[{k!r}]", X) for k in want}
    return period, listed, R, M, q, qd, count, prof


def _sample_result(ctx, q, qd, count, M, period, return_device):
    t = np.arange(M, dtype=np.float64) * period
    if return_device:
        for v in (q, qd, count):
            ctx.hand_over(v)
        return dict(q=q, qd=qd, count=count, t=t)
    return dict(q=ctx.to_host(q), qd=ctx.to_host(qd), count=ctx.to_host(count), t=t)


def _sample_rows(ctx, X, profile, period, rows, max_samples, return_device, blended):
    """The one sampler call behind sample_rows_on (edmp_sample_rows_dev) and sample_blended_rows_on (edmp_sample_blended_rows_dev: beta
    too, two times per waypoint).  X: the state on ctx's stream."""
    from . import _capi
    from .runtime import ptr

    n, N = X.shape[0], X.shape[2]
    # what the entry reads of the profile, in its argument order (limit and blend are reports, the samplers do not read them)
    want = dict(y=(n, N), phase=(n, N - 1, 3), times=(n, N, 2) if blended else (n, N), duration=(n,), seg=(n, N - 1, 2))
    if blended:
        want = dict(beta=(n, N), **want)
    entry = "edmp_sample_blended_rows_dev" if blended else "edmp_sample_rows_dev"
    period, listed, R, M, q, qd, count, prof = _sample_setup(ctx, X, want, profile, period, rows, max_samples)
    _capi.check(getattr(ctx.lib, entry)(ctx.h, ptr(X), n, N, *(ptr(prof[k]) for k in want), None if listed is None else _capi.as_pi32(listed),
                                        0 if listed is None else R, period, M, ptr(q), ptr(qd), ptr(count)), entry)
    return _sample_result(ctx, q, qd, count, M, period, return_device)


def sample_rows_on(ctx, trajectories, profile, period, rows=None, max_samples=None, return_device: bool = False) -> dict:
    """edmp_sample_rows_dev on the context `ctx` (runtime.Context): see sample_rows."""
    return _sample_rows(ctx, _rows_state(ctx, trajectories), profile, period, rows, max_samples, return_device, False)


def sample_rows(trajectories, profile, period, rows=None, max_samples=None, device="cuda:0", return_device: bool = False) -> dict:
    """The timed motion of the listed rows at a controller period (edmp_sample_rows_dev, csrc/timing.hip): trajectories (n, 7, N) and the
    `profile` time_rows gave for them, period [s] -> dict(q (R, 7, M) joint positions and qd (R, 7, M) joint velocities at t = k * period,
    count (R,) int32 = the samples of each row up to and including the first at rest at the goal (sample_count), t (M,)).  ``rows``: row
    indices in any order without duplicates, default every row; slot k of the outputs belongs to rows[k].  ``max_samples`` = M defaults to
    the largest count of the listed rows; a smaller value is refused, naming the row; more than 1048576 (EDMP_MAX_TIMED_SAMPLES) are refused
    by the library.  Every sample lies on its segment of the polyline; samples at or past count - 1 are the goal column bit for bit, at
    rest.  A row that was not timed gives NaN samples and count 0.  Runs on the GPU only."""
    from .runtime import get_context

    return sample_rows_on(get_context(device), trajectories, profile, period, rows, max_samples, return_device)


CERTIFY_VERDICT_NAMES = ("free", "hit", "undecided", "invalid")  # the codes of certify_rows' `verdict`; -1 = a row outside `rows`
BLEND_CODE_NAMES = ("none", "not_needed", "no_gain", "blended", "blocked")  # the codes of blend_rows' `code`; -1 = a row left alone


def blend_arguments(deviation, reach, substeps, halvings):
    """(deviation (7,) float64, reach, substeps, halvings) as edmp_blend_rows_dev takes them: a scalar deviation [rad] stands for all seven
    joints.  The library checks the ranges."""
    dev = np.ascontiguousarray(np.broadcast_to(np.asarray(deviation, dtype=np.float64), (7,)))
    return dev, float(reach), int(substeps), int(halvings)


def time_blended_rows_on(ctx, trajectories, beta, vmax=None, amax=None, jump=None, scale=(1, 1), return_device: bool = False) -> dict:
    """edmp_time_blended_rows_dev on the context `ctx` (runtime.Context): see time_blended_rows."""
    limits = franka.timing_limits(vmax, amax, jump, scale)
    X = _rows_state(ctx, trajectories)
    return _time_rows(ctx, X, _device_f64(ctx, beta, (X.shape[0], X.shape[2]), "beta", X), limits, return_device)


def time_blended_rows(trajectories, beta, vmax=None, amax=None, jump=None, scale=(1, 1), device="cuda:0", return_device: bool = False) -> dict:
    """Time every finished row along its BLENDED path (edmp_time_blended_rows_dev, csrc/timing.hip): trajectories (n, 7, N), 2 <= N <= 64,
    and beta (n, N) as blend_rows gave it (guide.blend_rows: corner i is replaced by the parabolic blend from x_i - beta_i d_{i-1} to
    x_i + beta_i d_i) -> time_rows' profile dict with two changes - times is (n, N, 2) = the time entering | leaving waypoint i's blend, and
    limit code 3 means "corner: jump cap or blend acceleration cap" - plus blend (n, N) = the time spent on each blend and beta itself,
    which sample_blended_rows reads.  The rule is time_rows' forward / backward pass with the blend's acceleration cap (2 beta_i) K_i as
    the corner cap and the straight part l_i = 1 - beta_i - beta_{i+1} as the segment; include/edmp_hip.h states it in full.  The
    velocity is continuous at a blended corner, |qdot| <= vmax and |qddot| <= amax hold on straight parts and on blends.  With beta = 0
    everywhere every common output has time_rows' bits.  A row with a non-finite element (of X or beta) is not timed.  Needs no scene
    and no guide.  Runs on the GPU only."""
    from .runtime import get_context

    return time_blended_rows_on(get_context(device), trajectories, beta, vmax, amax, jump, scale, return_device)


def sample_blended_rows_on(ctx, trajectories, profile, period, rows=None, max_samples=None, return_device: bool = False) -> dict:
    """edmp_sample_blended_rows_dev on the context `ctx` (runtime.Context): see sample_blended_rows."""
    return _sample_rows(ctx, _rows_state(ctx, trajectories), profile, period, rows, max_samples, return_device, True)


def sample_blended_rows(trajectories, profile, period, rows=None, max_samples=None, device="cuda:0", return_device: bool = False) -> dict:
    """The blended, timed motion of the listed rows at a controller period (edmp_sample_blended_rows_dev, csrc/timing.hip): trajectories
    (n, 7, N) and the `profile` time_blended_rows gave for them (it carries beta) -> sample_rows' dict(q, qd (R, 7, M), count (R,), t (M,)).
    On a straight part q = x_i + (beta_i + s) d_i; on blend i q = x_i + beta_i (u^2 d_i - (1 - u)^2 d_{i-1}) and qdot = sqrt y_i ((1 - u)
    d_{i-1} + u d_i), u the fraction of the blend's time.  ``rows``, ``max_samples``, count, the goal's bits at rest past the duration and
    the NaN row are sample_rows'.  With beta = 0 everywhere: sample_rows' bits.  Runs on the GPU only."""
    from .runtime import get_context

    return sample_blended_rows_on(get_context(device), trajectories, profile, period, rows, max_samples, return_device)


def ensemble_report(guides, batch_size_per_guide, volumes, success, metrics) -> list:
    """Which guide of the ensemble produced collision-free, short, smooth plans: one entry per guide slice of the batch.  Guide i of
    `guides` (the run cfg's guide numbers) owns rows [i * bpg, (i + 1) * bpg) (infer_serial.py:70-91); `batch_size_per_guide` may also
    be a sequence of per-guide row counts (the `total_rows` extension deals uneven blocks).  volumes (B,) = row_swept_volumes' output,
    success = success_rows' dict (collision_free, ok), metrics = batch_metrics' dict; host arrays.  Entry: guide, first_row, rows,
    rows_collision_free, rows_ok, best_row (batch index of the slice's first minimum swept volume), min_swept_volume, and mean / median
    (dicts over the four metrics) of the slice's collision-free rows, None when it has none."""
    guides = [int(g) for g in guides]
    counts = [int(batch_size_per_guide)] * len(guides) if np.ndim(batch_size_per_guide) == 0 else [int(c) for c in batch_size_per_guide]
    vol = np.asarray(volumes)
    free, ok = np.asarray(success["collision_free"], dtype=bool), np.asarray(success["ok"], dtype=bool)
    met = {k: np.asarray(metrics[k], dtype=np.float64) for k in METRIC_KEYS}
    if len(counts) != len(guides) or sum(counts) != vol.shape[0] or any(a.shape != vol.shape for a in (free, ok, *met.values())):
        raise ValueError(f"ensemble_report: {len(guides)} guides with rows {counts} do not tile (B,) = {vol.shape} arrays")
    out, r0 = [], 0
    for g, cnt in zip(guides, counts):
        sl = slice(r0, r0 + cnt)
        keep = free[sl]
        some = bool(keep.any())
        out.append(dict(guide=g, first_row=r0, rows=cnt, rows_collision_free=int(keep.sum()), rows_ok=int(ok[sl].sum()),
                        best_row=(r0 + int(np.argmin(vol[sl]))) if cnt else None, min_swept_volume=float(np.min(vol[sl])) if cnt else None,
                        mean={k: float(np.mean(met[k][sl][keep])) for k in METRIC_KEYS} if some else None,
                        median={k: float(np.median(met[k][sl][keep])) for k in METRIC_KEYS} if some else None))
        r0 += cnt
    return out


def format_ensemble_report(report) -> list:
    """one printable line per entry of ensemble_report"""
    lines = []
    for e in report:
        line = (f"  guide {e['guide']:>3}: rows {e['first_row']}..{e['first_row'] + e['rows'] - 1}, collision-free {e['rows_collision_free']}/{e['rows']}, "
                f"ok {e['rows_ok']}/{e['rows']}, best row {e['best_row']} (swept volume {e['min_swept_volume']:.4g})")
        if e["mean"] is not None:
            m, d = e["mean"], e["median"]
            line += (f"; collision-free rows: joint path {m['joint_path_length']:.3f} (median {d['joint_path_length']:.3f}), ee path {m['ee_path_length']:.3f} "
                     f"({d['ee_path_length']:.3f}), joint SPARC {m['joint_sparc']:.3f} ({d['joint_sparc']:.3f}), ee SPARC {m['ee_sparc']:.3f} ({d['ee_sparc']:.3f})")
        lines.append(line)
    return lines
