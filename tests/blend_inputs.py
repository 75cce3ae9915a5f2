"""The corner-blend stage's rule as plain Python loops in float64, its admission check and the inputs of its tests (test infrastructure, no
GPU needed).

The rule is the specification of blend_rows_kernel (edmp_amd/csrc/blend.hip) and of the blended instantiations of time_rows_kernel and
sample_rows_kernel (edmp_amd/csrc/timing.hip; include/edmp_hip.h states it), written from the definition with the success check's host twin as the judge - not from the kernels.  Python
floats are IEEE doubles and every operation below is rounded on its own.

    d_i = x_{i+1} - x_i,  Delta_i = d_i - d_{i-1};  V_i, A_i, J_i as in tests/timing_inputs.py;  K_i = min_j amax_j / |Delta_ij|
    corner i  code 0: a zero segment beside it, or Delta_i = 0;   code 1: not J_i^2 < min(V_{i-1}^2, V_i^2)  (the corner cap does not bind)
              beta0 = min(reach, min_j (4 deviation_j) / |Delta_ij|);  h = 0..H, beta = beta0 2^-h:
                  not (2 beta) K_i > J_i^2: code 2, stop;   q(u) = x_i + beta (u^2 d_i - (1 - u)^2 d_{i-1}) at u = k / K_b, k = 0..K_b, each
                  handed to oracle.success_oracle.success_rows as a row of ONE waypoint;  no hit: code 3, keep beta, halved = h, stop
              all H + 1 tries hit: code 4
    timing    l_i = (1 - beta_i) - beta_{i+1};  c_i = min(V_{i-1}^2, V_i^2, beta_i > 0 ? (2 beta_i) K_i : J_i^2);  the passes of time_rows with
              (2 A_i) l_i;  p_i = min(V_i^2, (y_i + y_{i+1}) / 2 + A_i l_i);  blend time (2 beta_i) / sqrt y_i;  times summed line 0, blend 1, ...
    motion    straight part: q = x_i + (beta_i + s) d_i;  blend: u = clamp(tau sqrt y_i / (2 beta_i)), q as above, qdot = sqrt y_i ((1 - u)
              d_{i-1} + u d_i)

A case is ADMITTED (admit) if the comparisons J^2 < min(V^2) and (2 beta) K > J^2 are nowhere within 1e-9 relative, if codes and halved are
the same with every obstacle's extents grown and shrunk by 1e-6 m, and if its blended profile passes timing_inputs.admit's rule (the two
smallest candidates of `limit` more than 1e-9 relative apart, exact zeros excepted).  Sample periods come from choose_period, which puts no
sample within 1e-9 of the duration of a piece boundary.

Roundings of the longest chain, R (gates(N)); a GPU value may differ from the rule's by 4 R 2^-53 of its scale:
    beta      4: d_i, d_{i-1}, Delta_i, the quotient (4 deviation and the power of two are exact)
    y         2 (N - 1) + 16: per transfer the product (2 A) l and the sum; in front of them l (2), A (2), the corner cap (beta 4, K 3, product 1),
              V^2 (3) and one to spare
    times     4 (N - 1) + 24: per waypoint three phase sums and the blend sum; the phase's own operations (square roots, quotients,
              differences) and the blend time in front of them"""
import math

import numpy as np

from edmp_amd import franka
from oracle import success_oracle as SO
from tests import repair_inputs as RI
from tests import sdf_reference as R
from tests import shortcut_inputs as SI
from tests import timing_inputs as TI

EXTENTS = SI.EXTENTS  # the link boxes of the test guides
INF = float("inf")
GAP = 1e-9    # admission: no comparison of the rule closer than this, relative
GROW = 1e-6   # metres, admission: the obstacles' extents grown and shrunk by this
LIMITS = TI.LIMITS
CODE_NAMES = ("none", "not_needed", "no_gain", "blended", "blocked")
_cache = {}


def _min(a, b):
    return b if b < a else a


def gates(N):
    """the roundings R of the longest chain of each quantity (the module docstring counts them)"""
    return dict(beta=4, y=2 * (N - 1) + 16, times=4 * (N - 1) + 24)


def hits(Q, obstacle_config, kinds):
    """the success check's test on each configuration of Q (M, 7) -> (M,) bool: a row of one waypoint is that configuration alone"""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 7)
    if Q.shape[0] == 0:
        return np.zeros(0, dtype=bool)
    return SO.success_rows(Q[:, :, None], obstacle_config, 1, kinds, EXTENTS)["first"] >= 0


def _gap(a, b):
    """relative distance of the two sides of a comparison"""
    if not (math.isfinite(a) and math.isfinite(b)):
        return INF
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else INF


def corner_terms(x, i, vmax, amax, jump):
    """what corner i of the row x (7, N) is made of: dp = d_{i-1}, d = d_i, zero-neighbour / flat flags, V_{i-1}^2, V_i^2, J_i^2, K_i"""
    dp = [float(x[j, i]) - float(x[j, i - 1]) for j in range(7)]
    d = [float(x[j, i + 1]) - float(x[j, i]) for j in range(7)]
    Vp = V = J = K = INF
    zp = z = flat = True
    dl = []
    for j in range(7):
        adp, ad, adl = abs(dp[j]), abs(d[j]), abs(d[j] - dp[j])
        dl.append(adl)
        if adp != 0.0:
            zp = False
            Vp = _min(Vp, float(vmax[j]) / adp)
        if ad != 0.0:
            z = False
            V = _min(V, float(vmax[j]) / ad)
        if adl != 0.0:
            flat = False
            J = _min(J, float(jump[j]) / adl)
            K = _min(K, float(amax[j]) / adl)
    return dict(dp=dp, d=d, dl=dl, zp=zp, z=z, flat=flat, V2p=Vp * Vp, V2=V * V, J2=J * J, K=K)


def blend_config(x, i, beta, u):
    """q(u) of corner i's blend, in the header's operation order"""
    uu = u * u
    w = 1.0 - u
    ww = w * w
    q = np.empty(7)
    for j in range(7):
        x0 = float(x[j, i])
        dp, d = x0 - float(x[j, i - 1]), float(x[j, i + 1]) - x0
        q[j] = x0 + beta * (uu * d - ww * dp)
    return q


def blend_row(x, obstacle_config, kinds, limits, deviation, reach, Kb, H, binding_only=True, gain_rule=True, ends=True):
    """the rule on one row x (7, N) -> dict(beta (N,), code (N,), halved (N,), tested, gaps = the relative gaps of every comparison made,
    tries = [(i, h, beta, hit per k)]).  binding_only / gain_rule / ends = False leave that step of the rule out (for the tests that show
    what each step is for; ends=False tests k = 1..K_b - 1 only)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[1]
    vmax, amax, jump = limits
    dev = np.broadcast_to(np.asarray(deviation, dtype=np.float64), (7,))
    if not np.isfinite(x).all():
        return dict(beta=np.full(N, np.nan), code=np.full(N, -1, dtype=np.int32), halved=np.zeros(N, dtype=np.int32), tested=0, gaps=[], tries=[])
    beta, code, halved = np.zeros(N), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    gaps, tries, pending = [], [], {}
    for i in range(1, N - 1):
        c = corner_terms(x, i, vmax, amax, jump)
        if c["zp"] or c["z"] or c["flat"]:
            continue
        vm = _min(c["V2p"], c["V2"])
        gaps.append(_gap(c["J2"], vm))
        if binding_only and not c["J2"] < vm:
            code[i] = 1
            continue
        b0 = float(reach)
        for j in range(7):
            if c["dl"][j] != 0.0:
                b0 = _min(b0, (4.0 * float(dev[j])) / c["dl"][j])
        pending[i] = (c, b0)
    tested = 0
    ks = list(range(Kb + 1)) if ends else list(range(1, Kb))
    scale = 1.0
    for h in range(H + 1):
        todo = []
        for i in sorted(pending):
            c, b0 = pending[i]
            b = b0 * scale
            gaps.append(_gap((2.0 * b) * c["K"], c["J2"]))
            if gain_rule and not (2.0 * b) * c["K"] > c["J2"]:
                code[i] = 2
                del pending[i]
                continue
            todo.append((i, b))
        if not todo:
            break
        Q = np.array([blend_config(x, i, b, float(k) / float(Kb)) for i, b in todo for k in ks]).reshape(-1, 7)
        hit = hits(Q, obstacle_config, kinds).reshape(len(todo), len(ks)) if ks else np.zeros((len(todo), 0), dtype=bool)
        for (i, b), hk in zip(todo, hit):
            tested += len(ks)
            tries.append((i, h, b, hk.copy()))
            if not hk.any():
                code[i], beta[i], halved[i] = 3, b, h
                del pending[i]
            elif h == H:
                code[i] = 4
                del pending[i]
        scale = scale * 0.5
    return dict(beta=beta, code=code, halved=halved, tested=tested, gaps=gaps, tries=tries)


def blend_rows(X, obstacle_config, kinds, limits, deviation, reach, Kb, H, **kw):
    """the rule for every row of X (n, 7, N): the arrays of edmp_blend_rows_dev plus `runs`, the per-row records.  obstacle_config / kinds
    may be per-row lists (a scene batch)"""
    X = np.asarray(X, dtype=np.float64)
    per_row = isinstance(obstacle_config, list)
    runs = [blend_row(x, obstacle_config[r] if per_row else obstacle_config, kinds[r] if per_row else kinds, limits, deviation, reach, Kb, H, **kw)
            for r, x in enumerate(X)]
    return dict(beta=np.stack([r["beta"] for r in runs]), code=np.stack([r["code"] for r in runs]), halved=np.stack([r["halved"] for r in runs]),
                tested=np.array([r["tested"] for r in runs], dtype=np.int32), runs=runs)


def time_blended_row(x, beta, vmax, amax, jump):
    """the blended profile of ONE row x (7, N) with beta (N,): dict(y (N,), phase (N-1, 3), times (N, 2), duration, limit (N,), seg (N-1, 2),
    blend (N,), cands (N, 6), ell (N-1,), V2, A, zero, beta)"""
    x, beta = np.asarray(x, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    N = x.shape[1]
    nan = float("nan")
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(beta))):
        return dict(y=np.full(N, nan), phase=np.full((N - 1, 3), nan), times=np.full((N, 2), nan), duration=nan, limit=np.full(N, -1, dtype=np.int32),
                    seg=np.full((N - 1, 2), nan), blend=np.full(N, nan), cands=np.full((N, 6), nan), beta=beta)
    d = [[float(x[j, i + 1]) - float(x[j, i]) for j in range(7)] for i in range(N - 1)]
    V2, A, zero, ell = [], [], [], []
    for i in range(N - 1):
        v, a, z = INF, INF, True
        for j in range(7):
            ad = abs(d[i][j])
            if ad != 0.0:
                z = False
                v = _min(v, float(vmax[j]) / ad)
                a = _min(a, float(amax[j]) / ad)
        V2.append(v * v)
        A.append(a)
        zero.append(z)
        ell.append((1.0 - float(beta[i])) - float(beta[i + 1]))
    cands = [[INF] * 6 for _ in range(N)]
    cands[0][0] = cands[N - 1][0] = 0.0
    c = [0.0] * N
    for i in range(1, N - 1):
        J = K = INF
        for j in range(7):
            den = abs(d[i][j] - d[i - 1][j])
            if den != 0.0:
                J = _min(J, float(jump[j]) / den)
                K = _min(K, float(amax[j]) / den)
        b = float(beta[i])
        cands[i][1], cands[i][2], cands[i][3] = V2[i - 1], V2[i], ((2.0 * b) * K if b > 0.0 else J * J)
        c[i] = _min(_min(cands[i][1], cands[i][2]), cands[i][3])
    y = [0.0] * N
    for i in range(N - 1):
        f = y[i] if zero[i] else y[i] + (2.0 * A[i]) * ell[i]
        y[i + 1] = _min(c[i + 1], f)
        if 0 < i + 1 < N - 1:
            cands[i + 1][4] = f
    for i in range(N - 2, -1, -1):
        b = y[i + 1] if zero[i] else y[i + 1] + (2.0 * A[i]) * ell[i]
        y[i] = _min(y[i], b)
        if 0 < i < N - 1:
            cands[i][5] = b
    limit = np.zeros(N, dtype=np.int32)
    for i in range(1, N - 1):
        best, code = INF, -1
        for k in range(1, 6):
            if cands[i][k] < best:
                best, code = cands[i][k], k
        limit[i] = code
    phase, seg, times, blend = np.zeros((N - 1, 3)), np.zeros((N - 1, 2)), np.zeros((N, 2)), np.zeros(N)
    t = 0.0
    for i in range(N - 1):
        if zero[i]:
            seg[i] = (0.0, y[i])
        else:
            p = (y[i] + y[i + 1]) / 2.0 + A[i] * ell[i]
            p = _min(p, V2[i])
            sp = math.sqrt(p)
            ta, td = (sp - math.sqrt(y[i])) / A[i], (sp - math.sqrt(y[i + 1])) / A[i]
            tc = ell[i] - (p - y[i]) / (2.0 * A[i]) - (p - y[i + 1]) / (2.0 * A[i])
            phase[i] = (ta if ta > 0.0 else 0.0, (tc if tc > 0.0 else 0.0) / sp, td if td > 0.0 else 0.0)
            seg[i] = (A[i], p)
        t = t + phase[i, 0]
        t = t + phase[i, 1]
        t = t + phase[i, 2]
        times[i + 1, 0] = t
        b = float(beta[i + 1])
        blend[i + 1] = (2.0 * b) / math.sqrt(y[i + 1]) if b > 0.0 else 0.0
        t = t + blend[i + 1]
        times[i + 1, 1] = t
    return dict(y=np.array(y), phase=phase, times=times, duration=float(t), limit=limit, seg=seg, blend=blend, cands=np.array(cands), ell=np.array(ell),
                V2=np.array(V2), A=np.array(A), zero=np.array(zero, dtype=bool), beta=beta)


def time_blended_rows(X, beta, vmax, amax, jump):
    """the rule for every row of X (n, 7, N) and beta (n, N): the arrays of edmp_time_blended_rows_dev"""
    rows = [time_blended_row(x, b, vmax, amax, jump) for x, b in zip(X, beta)]
    out = {k: np.stack([r[k] for r in rows]) for k in ("y", "phase", "times", "limit", "seg", "blend", "beta")}
    out["duration"] = np.array([r["duration"] for r in rows])
    out["rows"] = rows
    return out


def line_state(prof, i, tau, clamp=True):
    """(s, sdot) on the straight part of segment i at the time tau since it was entered; s counts from its start, 0..l_i"""
    ta, tc, _ = (float(v) for v in prof["phase"][i])
    A, p = (float(v) for v in prof["seg"][i])
    yi, y1, ell = float(prof["y"][i]), float(prof["y"][i + 1]), float(prof["ell"][i])
    sp = math.sqrt(p)
    if tau < ta:
        sy = math.sqrt(yi)
        sd, s = sy + A * tau, sy * tau + (0.5 * A) * (tau * tau)
    else:
        t2 = tau - ta
        if t2 < tc:
            sd, s = sp, (p - yi) / (2.0 * A) + sp * t2
        else:
            t3 = t2 - tc
            sd, s = sp - A * t3, (ell - (p - y1) / (2.0 * A)) + (sp * t3 - (0.5 * A) * (t3 * t3))
    if clamp:
        sd = sd if sd > 0.0 else 0.0
        sd = sd if sd < sp else sp
        s = s if s > 0.0 else 0.0
        s = s if s < ell else ell
    return s, sd


def blend_state(x, prof, i, tau, clamp=True):
    """(q, qdot, u) on blend i at the time tau since it was entered"""
    b, sy = float(prof["beta"][i]), math.sqrt(float(prof["y"][i]))
    u = (tau * sy) / (2.0 * b)
    if clamp:
        u = u if u > 0.0 else 0.0
        u = u if u < 1.0 else 1.0
    w = 1.0 - u
    q, qd = blend_config(x, i, b, u), np.empty(7)
    for j in range(7):
        x0 = float(x[j, i])
        dp, d = x0 - float(x[j, i - 1]), float(x[j, i + 1]) - x0
        qd[j] = sy * (w * dp + u * d)
    return q, qd, u


def motion(x, prof, t):
    """(q (7,), qdot (7,), piece, parameter) of the blended timed row at time t: piece p even = straight part of segment p / 2 (parameter
    beta_i + s), p odd = blend (p + 1) / 2 (parameter u); at or past the duration: the goal column itself, at rest"""
    N = x.shape[1]
    if not math.isfinite(prof["duration"]):
        return np.full(7, np.nan), np.full(7, np.nan), -1, float("nan")
    if t >= prof["duration"]:
        return x[:, N - 1].copy(), np.zeros(7), 2 * N - 4, 1.0
    F = prof["times"].reshape(-1)
    p = 0
    for m in range(2 * N - 3):  # the largest p with F[p + 1] <= t
        if float(F[m + 1]) <= t:
            p = m
    tau = t - float(F[p + 1])
    if p & 1:
        q, qd, u = blend_state(x, prof, (p + 1) >> 1, tau)
        return q, qd, p, u
    i = p >> 1
    s, sd = line_state(prof, i, tau)
    s = float(prof["beta"][i]) + s
    q, qd = np.empty(7), np.empty(7)
    for j in range(7):
        dj = float(x[j, i + 1]) - float(x[j, i])
        q[j] = float(x[j, i]) + s * dj
        qd[j] = dj * sd
    return q, qd, p, s


def sample_row(x, prof, period, M):
    """q, qd (7, M), the piece and parameter of every sample (M,), and the row's count"""
    q, qd, piece, par = np.empty((7, M)), np.empty((7, M)), np.empty(M, dtype=np.int64), np.empty(M)
    for k in range(M):
        q[:, k], qd[:, k], piece[k], par[k] = motion(x, prof, float(k) * period)
    return dict(q=q, qd=qd, piece=piece, parameter=par, count=TI.sample_count(prof["duration"], period))


def period_clear(profs, period, rel=1e-9):
    """no sample t_k = k period > 0 of any timed row within rel x duration of a piece boundary or of the duration"""
    for prof in profs:
        dur = prof["duration"]
        if not math.isfinite(dur) or dur == 0.0:
            continue
        F = np.unique(prof["times"].reshape(-1))
        F = F[F > 0.0]
        k = np.rint(F / period)
        if (np.abs(k * period - F) <= rel * dur).any():
            return False
    return True


def choose_period(profs, samples):
    """a period that gives about `samples` samples for the longest row (1 ms where nothing moves) and passes period_clear"""
    durs = [p["duration"] for p in profs if math.isfinite(p["duration"])]
    d = max(durs, default=0.0)
    base = float(d) / samples if d > 0 else 1e-3
    for m in range(64):
        period = base * (1.0 + 1e-3 * m)
        if period_clear(profs, period):
            return period
    raise AssertionError("no clear period")


def dense_check(x, prof, limits, deviation, dense=25):
    """the limit properties on a dense evaluation of the blended motion: the largest ratios speed = |qdot_j| / vmax_j and accel = |qddot_j| /
    amax_j (straight part: d_ij A_i in the accelerating phases; blend: y_i Delta_ij / (2 beta_i)), position and velocity discontinuity at
    every piece boundary (velocity relative to jump_j; at an unblended corner that is the jump ratio), deviation = the per-joint distance of a
    blend point from the matched point of the polyline over deviation_j, and how far the motion's end is from the goal at rest"""
    vmax, amax, jump = limits
    dev = np.broadcast_to(np.asarray(deviation, dtype=np.float64), (7,))
    N = x.shape[1]
    out = dict(speed=0.0, accel=0.0, position_gap=0.0, velocity_gap_blended=0.0, velocity_gap_unblended=0.0, deviation=0.0, end=0.0)
    beta, y = prof["beta"], prof["y"]
    prev = None  # (q, qd) at the end of the piece before
    for p in range(2 * N - 3):
        i = (p + 1) >> 1 if p & 1 else p >> 1
        if p & 1:
            T = float(prof["blend"][i])
            if T == 0.0:
                continue
            b = float(beta[i])
            dl = (x[:, i + 1] - x[:, i]) - (x[:, i] - x[:, i - 1])
            out["accel"] = max(out["accel"], float(np.max(np.abs(dl) * float(y[i]) / (2.0 * b) / amax)))
            first = last = None
            for tau in np.linspace(0.0, T, dense):
                q, qd, u = blend_state(x, prof, i, float(tau), clamp=False)
                out["speed"] = max(out["speed"], float(np.max(np.abs(qd) / vmax)))
                on = x[:, i] - b * (1.0 - 2.0 * u) * (x[:, i] - x[:, i - 1]) if u <= 0.5 else x[:, i] + b * (2.0 * u - 1.0) * (x[:, i + 1] - x[:, i])
                out["deviation"] = max(out["deviation"], float(np.max(np.abs(q - on) / dev)))
                first = first if first is not None else (q, qd)
                last = (q, qd)
        else:
            T = float(prof["phase"][i].sum())
            if T == 0.0:
                continue
            d = x[:, i + 1] - x[:, i]
            A, pk = float(prof["seg"][i, 0]), float(prof["seg"][i, 1])
            if prof["phase"][i, 0] > 0.0 or prof["phase"][i, 2] > 0.0:
                out["accel"] = max(out["accel"], float(np.max(np.abs(d) * A / amax)))
            first = last = None
            for tau in sorted(set(np.linspace(0.0, T, dense).tolist() + np.cumsum(prof["phase"][i]).tolist())):
                s, sd = line_state(prof, i, tau, clamp=False)
                q, qd = x[:, i] + (float(beta[i]) + s) * d, d * sd
                out["speed"] = max(out["speed"], float(np.max(np.abs(qd) / vmax)))
                first = first if first is not None else (q, qd)
                last = (q, qd)
        if prev is not None:
            out["position_gap"] = max(out["position_gap"], float(np.abs(first[0] - prev[0]).max()))
            gap = float(np.max(np.abs(first[1] - prev[1]) / jump))
            corner = i if p & 1 else i  # the waypoint between the two pieces, or the blend's own
            key = "velocity_gap_blended" if float(beta[corner]) > 0.0 else "velocity_gap_unblended"
            out[key] = max(out[key], gap)
        prev = last
    if prev is not None:
        out["end"] = max(float(np.abs(prev[0] - x[:, N - 1]).max()), float(np.abs(prev[1]).max()))
    return out


def grown(obstacle_config, by):
    oc = np.array(obstacle_config, dtype=np.float64)
    oc[:, 7:10] += by
    return oc


def admit(X, obstacle_config, kinds, limits, deviation, reach, Kb, H):
    """-> (admitted, reason, the rule's result, the blended profiles): no comparison within GAP, the same codes and halved with the extents
    grown and shrunk by GROW, and every profile admitted by timing_inputs.admit"""
    ref = blend_rows(X, obstacle_config, kinds, limits, deviation, reach, Kb, H)
    for r, run in enumerate(ref["runs"]):
        near = [g for g in run["gaps"] if g <= GAP]
        if near:
            return False, f"row {r}: a comparison within {near[0]!r} relative", ref, None
    per_row = isinstance(obstacle_config, list)
    for what, by in (("grown", GROW), ("shrunk", -GROW)):
        oc = [grown(o, by) for o in obstacle_config] if per_row else grown(obstacle_config, by)
        alt = blend_rows(X, oc, kinds, limits, deviation, reach, Kb, H)
        if not (np.array_equal(alt["code"], ref["code"]) and np.array_equal(alt["halved"], ref["halved"])):
            return False, f"other codes with the obstacles {what}", ref, None
    prof = time_blended_rows(X, ref["beta"], *limits)
    for r, p in enumerate(prof["rows"]):
        ok, worst = TI.admit(p)
        if not ok:
            return False, f"row {r}: limit candidates {worst!r} relative apart", ref, prof
    return True, "", ref, prof


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def far_obstacles(no, ncyl):
    """`no` obstacles >= 5 m away, the last `ncyl` of them cylinders: they fill the table and decide nothing"""
    inp = R.make_case(5, 1, 1, no, ncyl, far=True)
    return inp["obstacle_config"], inp["kinds"]


def with_far(obstacle_config, kinds, no, ncyl):
    """the deciding obstacles first, then far ones up to `no` in all, `ncyl` far cylinders among them (cuboids before cylinders is the
    loader's order, which nothing here needs: every obstacle carries its own kind)"""
    oc, kd = far_obstacles(no - len(kinds), ncyl) if no > len(kinds) else (np.zeros((0, 10)), np.zeros(0, dtype=np.int32))
    return np.ascontiguousarray(np.concatenate([obstacle_config, oc])), np.concatenate([kinds, kd]).astype(np.int32)


def l_corner():
    """ONE row of three waypoints: the mid configuration with joint 0 at -0.9 rad, the mid configuration, the mid configuration with joint 1 at
    +0.8 rad (two lengths: equal ones would tie V_0^2 with V_1^2).  The corner turns from joint 0 alone to joint 1 alone, so the blend (inside the triangle) carries the fingers to places that
    neither leg of the polyline visits.  With deviation 0.1 rad beta0 = min(0.4, 0.4 / 0.9) = 0.4."""
    lo, hi = franka.joint_limits()
    mid = (lo + hi) / 2
    a, c = mid.copy(), mid.copy()
    a[0], c[1] = -0.9, mid[1] + 0.8
    return np.ascontiguousarray(np.stack([a, mid, c], axis=1)[None])


L_DEVIATION, L_BETA0 = 0.1, 0.4


def middle_probe(cylinder=False):
    """a 2 cm cube (or a cylinder of radius 1 cm and height 2 cm) that the finger box reaches at the MIDDLE configuration u = 1/2 of the
    l_corner blend at beta0 alone: 4.5 cm (4.25 cm) beyond the finger's centre there, away from its place at the corner waypoint.  The
    polyline, the blend's other configurations at u = k / 4 and every configuration of the halved blend clear it (check_probes)."""
    x = l_corner()[0]
    _, c1 = SO.link_box_poses_batch(blend_config(x, 1, L_BETA0, 0.5)[None])
    _, c0 = SO.link_box_poses_batch(x[:, 1][None])
    v = c1[0, 8] - c0[0, 8]
    p = c1[0, 8] + (0.0425 if cylinder else 0.045) * v / np.linalg.norm(v)
    dims = (0.01, 0.01, 0.02) if cylinder else (0.02, 0.02, 0.02)
    return np.array([[p[0], p[1], p[2], 0.0, 0.0, 0.0, 1.0, *dims]]), np.full(1, 1 if cylinder else 0, dtype=np.int32)


def end_probe():
    """a 1 cm cube that link box 6 reaches at the END configuration u = 1 of the l_corner blend at beta0 alone - a point of the polyline,
    0.4 of the way along the second segment, between the success check's substeps 0.25 and 0.5 - 5.5 cm from that box's centre along its first axis"""
    x = l_corner()[0]
    Rl, cl = SO.link_box_poses_batch(blend_config(x, 1, L_BETA0, 1.0)[None])
    p = cl[0, 6] + 0.055 * Rl[0, 6][:, 0]
    return np.array([[p[0], p[1], p[2], 0.0, 0.0, 0.0, 1.0, 0.01, 0.01, 0.01]]), np.zeros(1, dtype=np.int32)


def check_probes():
    """asserts on the CPU what the probes' docstrings say -> dict of the hit patterns"""
    x = l_corner()[0]
    poly = np.array([(1 - f) * x[:, i] + f * x[:, i + 1] for i in range(2) for f in np.linspace(0, 1, 65)])
    succ = np.array([(1 - f) * x[:, i] + f * x[:, i + 1] for i in range(2) for f in (0, 0.25, 0.5, 0.75, 1)])
    full = np.array([blend_config(x, 1, L_BETA0, k / 8) for k in range(9)])
    half = np.array([blend_config(x, 1, L_BETA0 / 2, k / 8) for k in range(9)])
    out = {}
    for name, (oc, kd) in (("cube", middle_probe()), ("cylinder", middle_probe(True))):
        h = hits(full, oc, kd)
        assert h[4] and not h[[0, 2, 6, 8]].any() and not hits(half, oc, kd).any() and not hits(poly, oc, kd).any(), name
        out[name] = h
    oc, kd = end_probe()
    h = hits(full, oc, kd)
    assert h[8] and not h[[0, 2, 4, 6]].any() and not hits(half, oc, kd).any() and not hits(succ, oc, kd).any()
    out["end"] = h
    return out


def _limits(**kw):
    return tuple(np.asarray(v, dtype=np.float64) for v in franka.timing_limits(**kw))


def gentle_rows(seed, n):
    """rows of three waypoints whose middle one lies 1e-3 of the way off the chord's midpoint: the jump cap does not bind (not needed)"""
    X = TI.coarse_rows(seed, n, 3)
    rs = np.random.RandomState(seed + 1)
    X[:, :, 1] = (X[:, :, 0] + X[:, :, 2]) / 2 + 1e-3 * rs.uniform(-1, 1, size=(n, 7)) * (X[:, :, 2] - X[:, :, 0])
    return X


def _random_scene(seed, no, ncyl):
    inp = R.make_case(seed, 1, 1, no, ncyl)
    return inp["obstacle_config"], inp["kinds"]


def _build():
    L = l_corner()
    far1 = far_obstacles(1, 0)
    x = L[0]
    c = corner_terms(x, 1, *LIMITS)
    # h = 0 is tried (and hits the probe), h = 1 is no gain: J^2 = 1.5 beta0 K lies between (2 beta0) K and (2 beta0 / 2) K
    jt = math.sqrt(1.5 * L_BETA0 * c["K"])
    gain_jump = _limits(jump=np.full(7, jt * max(c["dl"])))
    big_jump = _limits(jump=np.asarray(franka.JOINT_VELOCITY_LIMITS) * 100.0)
    mid_jump = _limits(jump=np.asarray(franka.JOINT_VELOCITY_LIMITS) * 0.05)
    two = TI.coarse_rows(3, 2, 2)
    still = np.repeat(TI.coarse_rows(5, 1, 1), 5, axis=2)
    nan = TI.walk_rows(17, 3, 50)
    nan[1, 3, 20] = np.nan
    base = dict(limits=LIMITS, deviation=0.01, reach=0.4, Kb=4, H=2)
    cases = {
        "L_free_blended_at_h0": dict(base, X=L, scene=far1, deviation=L_DEVIATION),
        "L_middle_decides_h1_passes": dict(base, X=L, scene=middle_probe(), deviation=L_DEVIATION),
        "L_middle_decides_H0_blocked": dict(base, X=L, scene=middle_probe(), deviation=L_DEVIATION, H=0),
        "L_middle_untested_at_K1": dict(base, X=L, scene=middle_probe(), deviation=L_DEVIATION, Kb=1),
        "L_middle_cylinder_o7_K8_H3": dict(base, X=L, scene=with_far(*middle_probe(True), 7, 2), deviation=L_DEVIATION, Kb=8, H=3),
        "L_end_decides_o64": dict(base, X=L, scene=with_far(*end_probe(), 64, 8), deviation=L_DEVIATION, H=1),
        "L_no_gain_at_h0": dict(base, X=L, scene=far1, deviation=1e-9),
        "L_hit_then_no_gain_at_h1": dict(base, X=L, scene=middle_probe(), deviation=L_DEVIATION, limits=gain_jump, H=3),
        "gentle_N3_n7_not_needed": dict(base, X=gentle_rows(21, 7), scene=_random_scene(2, 7, 2)),
        "walk_N50_n9_o7c2": dict(base, X=TI.walk_rows(11, 9, 50), scene=_random_scene(1, 7, 2)),
        "walk_N64_n5_o64c8_K8_H3": dict(base, X=TI.walk_rows(12, 5, 64), scene=with_far(*_random_scene(1, 7, 2), 64, 8), deviation=0.05, Kb=8, H=3),
        "walk_N64_n5_big_jump_not_needed": dict(base, X=TI.walk_rows(12, 5, 64), scene=far1, limits=big_jump),
        "coarse_N4_n4_o1_K1": dict(base, X=TI.coarse_rows(13, 4, 4), scene=_random_scene(3, 1, 0), deviation=0.05, Kb=1, H=1),
        "coarse_N5_n6_o7c2_H3": dict(base, X=TI.coarse_rows(19, 6, 5), scene=_random_scene(6, 7, 2), deviation=0.2, H=3),
        "pair_N4_n8_both_at_reach_045": dict(base, X=TI.coarse_rows(14, 8, 4), scene=far1, deviation=10.0, reach=0.45),
        "two_N2_n2": dict(base, X=two, scene=far1),
        "zeros_N8_n3_start_middle_pair": dict(base, X=TI.with_zero_segments(TI.walk_rows(15, 3, 8, 0.3), [[(0, 1)], [(3, 1)], [(2, 2)]]), scene=far1, limits=mid_jump,
                                              deviation=0.05),
        "still_N5_n1": dict(base, X=still, scene=far1),
        "chord_N50_n1_collinear_run": dict(base, X=TI.chord_row(16, 50, 6, 45, 0.2), scene=far1),
        "nan_N50_n3": dict(base, X=nan, scene=_random_scene(1, 7, 2)),
    }
    return cases


def names():
    return ["L_free_blended_at_h0", "L_middle_decides_h1_passes", "L_middle_decides_H0_blocked", "L_middle_untested_at_K1", "L_middle_cylinder_o7_K8_H3",
            "L_end_decides_o64", "L_no_gain_at_h0", "L_hit_then_no_gain_at_h1", "gentle_N3_n7_not_needed", "walk_N50_n9_o7c2", "walk_N64_n5_o64c8_K8_H3",
            "walk_N64_n5_big_jump_not_needed", "coarse_N4_n4_o1_K1", "coarse_N5_n6_o7c2_H3", "pair_N4_n8_both_at_reach_045", "two_N2_n2",
            "zeros_N8_n3_start_middle_pair", "still_N5_n1", "chord_N50_n1_collinear_run", "nan_N50_n3"]


# what the named cases must show (test_blend_host.py: test_case_conditions checks each on the CPU)
EXPECT = {
    "L_free_blended_at_h0": dict(code=[[0, 3, 0]], halved=[[0, 0, 0]], tested=[5]),
    "L_middle_decides_h1_passes": dict(code=[[0, 3, 0]], halved=[[0, 1, 0]], tested=[10]),
    "L_middle_decides_H0_blocked": dict(code=[[0, 4, 0]], halved=[[0, 0, 0]], tested=[5]),
    "L_middle_untested_at_K1": dict(code=[[0, 3, 0]], halved=[[0, 0, 0]], tested=[2]),
    "L_middle_cylinder_o7_K8_H3": dict(code=[[0, 3, 0]], halved=[[0, 1, 0]], tested=[18]),
    "L_end_decides_o64": dict(code=[[0, 3, 0]], halved=[[0, 1, 0]], tested=[10]),
    "L_no_gain_at_h0": dict(code=[[0, 2, 0]], halved=[[0, 0, 0]], tested=[0]),
    "L_hit_then_no_gain_at_h1": dict(code=[[0, 2, 0]], halved=[[0, 0, 0]], tested=[5]),
}


def case(name):
    """a case with its references: X (n, 7, N), obstacle_config, kinds, limits, deviation, reach, Kb, H, ref = blend_rows(...), prof =
    time_blended_rows(X, ref beta, ...), cfgs.  Built once, shared, never written to; every case is admitted (asserted here)."""
    if name not in _cache:
        if "_built" not in _cache:
            built = _build()
            assert list(built) == names()
            _cache["_built"] = built
        c = dict(_cache["_built"][name])
        c["obstacle_config"], c["kinds"] = c.pop("scene")
        ok, why, ref, prof = admit(c["X"], c["obstacle_config"], c["kinds"], c["limits"], c["deviation"], c["reach"], c["Kb"], c["H"])
        assert ok, f"{name}: not admitted: {why}"
        c["X"].setflags(write=False)
        c.update(name=name, ref=ref, prof=prof, cfgs=RI.plain_cfgs(c["X"].shape[0]))
        _cache[name] = c
    return _cache[name]


def call_args(c):
    """the keyword arguments of guide.blend_rows for a case"""
    vmax, amax, jump = c["limits"]
    return dict(deviation=c["deviation"], reach=c["reach"], substeps=c["Kb"], halvings=c["H"], vmax=vmax, amax=amax, jump=jump)


# ---- the input families of the informative duration table and of the binding-only rule's test ---------------------------------------------
def knot_rows(seed, n, knots=5):
    """what shortcutting leaves: a few far-apart configurations"""
    return TI.coarse_rows(seed, n, knots)


def collinear_rows(seed, n, N=50, knots=5):
    """knot_rows sampled to N waypoints along its polyline: runs of collinear waypoints whose Delta is a rounding, between a few real corners"""
    Kn = knot_rows(seed, n, knots)
    X = np.empty((n, 7, N))
    for m, t in enumerate(np.linspace(0.0, knots - 1.0, N)):
        i = min(int(t), knots - 2)
        X[:, :, m] = Kn[:, :, i] + (t - i) * (Kn[:, :, i + 1] - Kn[:, :, i])
    X[:, :, 0], X[:, :, -1] = Kn[:, :, 0], Kn[:, :, -1]
    return X


def families(n=8):
    """name -> rows (n, 7, N): the families whose durations before and after blending test_blend_host.py prints"""
    g = RI.graze_scene(0.0)
    return {"noisy smooth 50-waypoint rows": TI.walk_rows(41, n, 50, 0.01), "bumped zigzag rows": SI.zigzag_rows(g["start"], g["goal"], 50, min(n, 6)),
            "5-knot rows": knot_rows(42, n), "5-knot rows sampled to 50 collinear waypoints": collinear_rows(42, n)}
