"""The time parameterisation's rule as plain Python loops in float64, its admission check and the inputs of its tests (test infrastructure,
no GPU needed).

The rule is the specification of time_rows_kernel and sample_rows_kernel (edmp_amd/csrc/timing.hip; include/edmp_hip.h states it), written
from the definition - not from the kernels.  Python floats are IEEE doubles and every operation below is rounded on its own, so the rule's
numbers are what a faithful device statement gives, up to the order of operations the header fixes.

    segment i    d_i = x_{i+1} - x_i;  V_i = min_j vmax_j / |d_ij|,  A_i = min_j amax_j / |d_ij| over d_ij != 0;  d_i = 0: a zero segment
    waypoint i   c_0 = c_{N-1} = 0;  c_i = min(V_{i-1}^2, V_i^2, J_i^2),  J_i = min_j jump_j / |d_ij - d_{i-1,j}|, absent terms left out
    forward      y_0 = 0,  y_{i+1} = min(c_{i+1}, y_i + 2 A_i)        (zero segment: min(c_{i+1}, y_i))
    backward     y_i = min(y_i, y_{i+1} + 2 A_i)                       (zero segment: min(y_i, y_{i+1}))
    segment      p_i = min(V_i^2, (y_i + y_{i+1}) / 2 + A_i);  accelerate, cruise, decelerate;  times summed in index order
    limit_i      first index of the minimum among rest | V_{i-1}^2 | V_i^2 | J_i^2 | forward candidate | backward candidate

A case is ADMITTED (admit) if at every interior waypoint the smallest and the second-smallest candidate of `limit` differ by more than
1e-9 relative: then no code sits on a rounding.  One kind of tie is admitted: candidates that are exactly 0.  A zero is only ever the rest
end's y = 0 handed across zero segments by min(), no operation rounds on the way, so host and device hold the same bits and the first index
decides on both (a row with start = goal throughout consists of nothing else)."""
import math

import numpy as np

from edmp_amd import franka

INF = float("inf")
GAP = 1e-9
LIMITS = tuple(np.asarray(v, dtype=np.float64) for v in franka.timing_limits())
_cache = {}


def _min(a, b):
    return b if b < a else a


def time_row(x, vmax, amax, jump, corner=True, backward=True, cruise=True):
    """the profile of ONE row x (7, N): dict(y (N,), phase (N-1, 3), times (N,), duration, limit (N,), seg (N-1, 2), cands (N, 6), V2, A,
    zero).  corner / backward / cruise = False leave that step of the rule out (for the tests that show what each step is for)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[1]
    nan = float("nan")
    if not np.all(np.isfinite(x)):
        return dict(y=np.full(N, nan), phase=np.full((N - 1, 3), nan), times=np.full(N, nan), duration=nan, limit=np.full(N, -1, dtype=np.int32),
                    seg=np.full((N - 1, 2), nan), cands=np.full((N, 6), nan))
    d = [[float(x[j, i + 1]) - float(x[j, i]) for j in range(7)] for i in range(N - 1)]
    V2, A, zero = [], [], []
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
    cands = [[INF] * 6 for _ in range(N)]
    cands[0][0] = cands[N - 1][0] = 0.0
    c = [0.0] * N
    for i in range(1, N - 1):
        J = INF
        for j in range(7):
            den = abs(d[i][j] - d[i - 1][j])
            if den != 0.0:
                J = _min(J, float(jump[j]) / den)
        cands[i][1], cands[i][2], cands[i][3] = V2[i - 1], V2[i], (J * J if corner else INF)
        c[i] = _min(_min(cands[i][1], cands[i][2]), cands[i][3])
    y = [0.0] * N
    for i in range(N - 1):
        f = y[i] if zero[i] else y[i] + 2.0 * A[i]
        y[i + 1] = _min(c[i + 1], f)
        if 0 < i + 1 < N - 1:
            cands[i + 1][4] = f
    if backward:
        for i in range(N - 2, -1, -1):
            b = y[i + 1] if zero[i] else y[i + 1] + 2.0 * A[i]
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
    phase, seg, times = np.zeros((N - 1, 3)), np.zeros((N - 1, 2)), np.zeros(N)
    t = 0.0
    for i in range(N - 1):
        if zero[i]:
            seg[i] = (0.0, y[i])
        else:
            p = (y[i] + y[i + 1]) / 2.0 + A[i]
            if cruise:
                p = _min(p, V2[i])
            sp = math.sqrt(p)
            ta, td = (sp - math.sqrt(y[i])) / A[i], (sp - math.sqrt(y[i + 1])) / A[i]
            tc = 1.0 - (p - y[i]) / (2.0 * A[i]) - (p - y[i + 1]) / (2.0 * A[i])
            phase[i] = (ta if ta > 0.0 else 0.0, (tc if tc > 0.0 else 0.0) / sp, td if td > 0.0 else 0.0)
            seg[i] = (A[i], p)
        t = t + phase[i, 0]
        t = t + phase[i, 1]
        t = t + phase[i, 2]
        times[i + 1] = t
    return dict(y=np.array(y), phase=phase, times=times, duration=float(t), limit=limit, seg=seg, cands=np.array(cands), V2=np.array(V2), A=np.array(A),
                zero=np.array(zero, dtype=bool))


def time_rows(X, vmax, amax, jump):
    """the rule for every row of X (n, 7, N): the arrays of edmp_time_rows_dev"""
    rows = [time_row(x, vmax, amax, jump) for x in X]
    out = {k: np.stack([r[k] for r in rows]) for k in ("y", "phase", "times", "limit", "seg")}
    out["duration"] = np.array([r["duration"] for r in rows])
    out["rows"] = rows
    return out


def segment_state(prof, i, tau, clamp=True):
    """(s, sdot) of segment i at the time tau since waypoint i: the closed-form quadratic of the phase that contains tau"""
    ta, tc, _ = (float(v) for v in prof["phase"][i])
    A, p = (float(v) for v in prof["seg"][i])
    yi, y1 = float(prof["y"][i]), float(prof["y"][i + 1])
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
            sd, s = sp - A * t3, (1.0 - (p - y1) / (2.0 * A)) + (sp * t3 - (0.5 * A) * (t3 * t3))
    if clamp:
        sd = sd if sd > 0.0 else 0.0
        sd = sd if sd < sp else sp
        s = s if s > 0.0 else 0.0
        s = s if s < 1.0 else 1.0
    return s, sd


def motion(x, prof, t):
    """(q (7,), qdot (7,), segment index, s) of the timed row at time t; at or past the duration: the goal column itself, at rest"""
    N = x.shape[1]
    if not math.isfinite(prof["duration"]):
        return np.full(7, np.nan), np.full(7, np.nan), -1, float("nan")
    if t >= prof["duration"]:
        return x[:, N - 1].copy(), np.zeros(7), N - 2, 1.0
    i = 0
    for m in range(N - 1):  # the largest i <= N - 2 with T_i <= t
        if float(prof["times"][m]) <= t:
            i = m
    s, sd = segment_state(prof, i, t - float(prof["times"][i]))
    q, qd = np.empty(7), np.empty(7)
    for j in range(7):
        dj = float(x[j, i + 1]) - float(x[j, i])
        q[j] = float(x[j, i]) + s * dj
        qd[j] = dj * sd
    return q, qd, i, s


def sample_count(duration, period):
    """1 + the smallest k with float(k) * period >= duration; 0 for a row that was not timed"""
    if not math.isfinite(duration):
        return 0
    g = int(math.ceil(duration / period))
    k = max(g - 2, 0)  # (the quotient is one rounding away from the truth: the smallest k is found by walking up from below it)
    while float(k) * period < duration:
        k += 1
    while k > 0 and float(k - 1) * period >= duration:
        k -= 1
    return 1 + k


def sample_row(x, prof, period, M):
    """q, qd (7, M), the segment index and s of every sample (M,), and the row's count"""
    q, qd, seg, s = np.empty((7, M)), np.empty((7, M)), np.empty(M, dtype=np.int64), np.empty(M)
    for k in range(M):
        q[:, k], qd[:, k], seg[k], s[k] = motion(x, prof, float(k) * period)
    return dict(q=q, qd=qd, segment=seg, s=s, count=sample_count(prof["duration"], period))


def admit(prof):
    """(admitted, the smallest relative gap between the two smallest candidates of an interior waypoint) of a row's profile"""
    worst = INF
    if not math.isfinite(prof["duration"]):
        return True, worst
    for i in range(1, len(prof["y"]) - 1):
        c = sorted(float(v) for v in prof["cands"][i])
        if c[0] == 0.0 and c[1] == 0.0:  # the rest end handed across zero segments on both sides: exact on host and device
            continue
        gap = (c[1] - c[0]) / c[1] if math.isfinite(c[1]) else INF
        worst = min(worst, gap)
    return worst > GAP, worst


def violations(x, prof, vmax, amax, jump, dense=48):
    """the limit properties on a dense evaluation of the timed row: the largest ratios speed = |qdot_j| / vmax_j, accel = |delta qdot_j| /
    (delta t amax_j) between neighbouring instants of one segment, jump = |d_ij - d_{i-1,j}| sqrt y_i / jump_j at the waypoints, and closure =
    how far a segment's motion is, at its first and last instant, from s = 0 at sqrt y_i and s = 1 at sqrt y_{i+1} (relative to 1 and to
    the segment's peak speed).
    All are <= 1 resp. ~ 0 for the rule."""
    N = x.shape[1]
    out = dict(speed=0.0, accel=0.0, jump=0.0, closure=0.0)
    for i in range(N - 1):
        if i > 0:
            for j in range(7):
                dd = abs((float(x[j, i + 1]) - float(x[j, i])) - (float(x[j, i]) - float(x[j, i - 1])))
                out["jump"] = max(out["jump"], dd * math.sqrt(float(prof["y"][i])) / float(jump[j]))
        total = float(prof["phase"][i].sum())
        if total == 0.0:
            continue
        d = np.array([float(x[j, i + 1]) - float(x[j, i]) for j in range(7)])
        ts = sorted(set(np.linspace(0.0, total, dense).tolist() + np.cumsum(prof["phase"][i]).tolist()))
        prev = None
        for tau in ts:
            s, sd = segment_state(prof, i, tau, clamp=False)
            out["speed"] = max(out["speed"], float(np.max(np.abs(d) * sd / vmax)))
            if prev is not None and tau > prev[0]:
                out["accel"] = max(out["accel"], float(np.max(np.abs(d) * abs(sd - prev[1]) / ((tau - prev[0]) * amax))))
            prev = (tau, sd)
        sp = math.sqrt(float(prof["seg"][i, 1]))
        s0, sd0 = segment_state(prof, i, 0.0, clamp=False)
        out["closure"] = max(out["closure"], abs(s0), abs(sd0 - math.sqrt(float(prof["y"][i]))) / sp, abs(s - 1.0), abs(sd - math.sqrt(float(prof["y"][i + 1]))) / sp)
    return out


# ---- seeded case builders -------------------------------------------------------------------------------------------------------------
def _ends(rs):
    lo, hi = franka.joint_limits()
    return rs.uniform(lo + 0.2, hi - 0.2), rs.uniform(lo + 0.2, hi - 0.2)


def walk_rows(seed, n, N, step=0.08, span=None):
    """sampler-like rows: the straight line start -> goal plus a random walk pinned at both ends; span: the largest joint displacement
    start -> goal, default whatever the two random configurations give"""
    rs = np.random.RandomState(seed)
    X = np.empty((n, 7, N))
    for r in range(n):
        a, b = _ends(rs)
        if span is not None:
            b = a + (b - a) * (span / np.abs(b - a).max())
        w = np.cumsum(rs.standard_normal((7, N)) * step, axis=1)
        w = w - np.linspace(0, 1, N)[None] * (w[:, -1:] - w[:, :1]) - w[:, :1]
        X[r] = a[:, None] + np.linspace(0, 1, N)[None] * (b - a)[:, None] + w
    return X


def coarse_rows(seed, n, N):
    """a few far-apart random configurations: long segments with a cruise phase"""
    rs = np.random.RandomState(seed)
    lo, hi = franka.joint_limits()
    return rs.uniform(lo[None, :, None] + 0.1, hi[None, :, None] - 0.1, size=(n, 7, N))


def chord_row(seed, N, i, j, span):
    """a walk row whose waypoints between i and j were replaced by the shortcut rule's piece y_m = x_i + ((m - i) / (j - i)) (x_j - x_i).
    (The chord must stay too short to reach its cruise speed: on a collinear run V_{i-1}^2 and V_i^2 differ by roundings only, and a
    waypoint bound by them is not admitted.)"""
    X = walk_rows(seed, 1, N, 0.02, span)
    for m in range(i + 1, j):
        g = float(m - i) / float(j - i)
        for k in range(7):
            X[0, k, m] = X[0, k, i] + g * (X[0, k, j] - X[0, k, i])
    return X


def with_zero_segments(X, spec):
    """row r of X with the waypoints spec[r] = [(m, count), ...] repeated: waypoints m+1..m+count become copies of waypoint m"""
    X = X.copy()
    for r, reps in enumerate(spec):
        for m, cnt in reps:
            X[r, :, m + 1:m + 1 + cnt] = X[r, :, m:m + 1]
    return X


def _limits(vmax=None, amax=None, jump=None, scale=(1.0, 1.0)):
    return tuple(np.asarray(v, dtype=np.float64) for v in franka.timing_limits(vmax, amax, jump, scale))


def _build():
    big_jump = _limits(jump=np.asarray(franka.JOINT_VELOCITY_LIMITS) * 100.0)  # corners cap nothing: velocity and acceleration bind
    mid_jump = _limits(jump=np.asarray(franka.JOINT_VELOCITY_LIMITS) * 0.05)
    two = coarse_rows(3, 2, 2)
    two[1] = two[0]
    two[1][:, 1] = two[0][:, 0] + 0.01 * (two[0][:, 1] - two[0][:, 0])  # row 0: a long segment that cruises; row 1: a short, triangular one
    still = np.repeat(coarse_rows(5, 1, 1), 5, axis=2)
    nan = walk_rows(17, 3, 50)
    nan[1, 3, 20] = np.nan
    cases = {
        "walk_N50_n9": dict(X=walk_rows(11, 9, 50), limits=LIMITS),
        "walk_N64_n5_big_jump": dict(X=walk_rows(12, 5, 64), limits=big_jump),
        "coarse_N4_n4_big_jump": dict(X=coarse_rows(13, 4, 4), limits=big_jump),
        "coarse_N3_n3": dict(X=coarse_rows(14, 3, 3), limits=mid_jump),
        "two_N2_n2_cruise_and_triangle": dict(X=two, limits=LIMITS),
        "zeros_N8_n3_start_middle_pair": dict(X=with_zero_segments(walk_rows(15, 3, 8, 0.3), [[(0, 1)], [(3, 1)], [(2, 2)]]), limits=mid_jump),
        "still_N5_n1": dict(X=still, limits=LIMITS),
        "still_N2_n1": dict(X=still[:, :, :2].copy(), limits=LIMITS),
        "chord_N50_n1": dict(X=chord_row(16, 50, 6, 45, 0.2), limits=LIMITS),
        "nan_N50_n3": dict(X=nan, limits=LIMITS),
    }
    return cases


def names():
    return ["walk_N50_n9", "walk_N64_n5_big_jump", "coarse_N4_n4_big_jump", "coarse_N3_n3", "two_N2_n2_cruise_and_triangle", "zeros_N8_n3_start_middle_pair",
            "still_N5_n1", "still_N2_n1", "chord_N50_n1", "nan_N50_n3"]


def case(name):
    """a case with its reference: X (n, 7, N), limits (vmax, amax, jump), ref = time_rows(...).  Built once, shared, never written to."""
    if not _cache:
        built = _build()
        assert list(built) == names()
        for k, c in built.items():
            c["ref"] = time_rows(c["X"], *c["limits"])
            c["X"].setflags(write=False)
            _cache[k] = c
    return _cache[name]
