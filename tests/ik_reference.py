"""An independent high-precision reference of the IK iteration, and the gates the step-by-step tests use - none of it is code under test.

* `mp_iterate`: the damped-least-squares step of include/edmp_hip.h in mpmath at 50 digits.  The FK is built from franka.DH_A_D_ALPHA,
  evaluation.EE_STATIC_DH (or a given tool matrix) and franka.joint_limits() only; the Jacobian is NOT the geometric z x (p_e - p_j) of
  csrc/ik.hip and tests/ik_inputs.dls_numpy but the derivative of that FK (central differences, h = 1e-20: truncation ~ h^2, rounding
  ~ 1e-50 / h), position rows dp/dq_j, rotation rows vee((dR/dq_j) R^T).  A lever arm, sign or frame mistake shared by the kernel and the
  NumPy restatement cannot hide behind it.
* `dls_cholesky`: a second f64 formulation of the iteration (joint rotations and origins accumulated separately, the Gram matrix summed
  joint by joint in reverse order, an unrolled Cholesky solve).  Its distance from dls_numpy is the noise floor of a correct f64
  implementation.
* `floors(setting)`: floor_mp[k] = max |dls_numpy - mpmath| on a subset, floor_f64[k] = max |dls_numpy - dls_cholesky| on every row,
  gate[k] = 100 x floor_f64[k], gate_mp[k] = 100 x max(floor_mp[k], floor_f64[k]) - computed when asked, cached per process.  The factor
  100 covers another sincos, FMA contraction and the kernel's own Cholesky; it can be generous because each mistake the gates are there
  to catch moves q by >= 3e-5 rad after one step (tests/test_ik_reference_host.py shows it for every mutant of dls_numpy).
"""
import functools

import numpy as np
from mpmath import mp, mpf

from edmp_amd import evaluation, franka
from tests import ik_inputs as I

DPS = 50
H = mpf(10) ** -20
MARGIN = 100.0
FULL_KS = (1, 2, 4, 8, 16)
MP_KS = (1, 2, 4)
SPECIAL_KS = (1, 2, 3)
SPECIAL_TARGETS = (0, 5)
MP_SEEDS_PER_TARGET = 8
SETTING_KS = (1, 4)
SETTING_TARGETS, SETTING_SEEDS, SETTING_MP_SEEDS = 3, 64, 4


def custom_tool() -> np.ndarray:
    """the rotated and offset frame of tests/test_gpu_ik.py::test_tool_frames"""
    custom = np.eye(4)
    c, s = np.cos(0.7), np.sin(0.7)
    custom[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    custom[:3, 3] = [0.02, -0.03, 0.15]
    return custom


SETTINGS = {
    "default": dict(tool=None, damping=I.DAMPING, max_step=I.MAX_STEP),
    "damped_small_steps": dict(tool=None, damping=0.1, max_step=0.05),  # every row scaled
    "light_large_steps": dict(tool=None, damping=1e-3, max_step=2.0),  # almost none scaled
    "flange": dict(tool="flange", damping=I.DAMPING, max_step=I.MAX_STEP),
    "custom": dict(tool=custom_tool(), damping=I.DAMPING, max_step=I.MAX_STEP),
}


# ---- mpmath -------------------------------------------------------------------------------------------------------------------------


def _eye():
    return [[mpf(int(a == b)) for b in range(4)] for a in range(4)]


def _mul(A, B):
    return [[A[a][0] * B[0][b] + A[a][1] * B[1][b] + A[a][2] * B[2][b] + A[a][3] * B[3][b] for b in range(4)] for a in range(4)]


def _mp_dh(a, d, alpha, theta):
    """one modified-DH row: Rot_x(alpha) Trans_x(a) Rot_z(theta) Trans_z(d)"""
    a, d, alpha, theta = mpf(a), mpf(d), mpf(alpha), mpf(theta)
    ct, st, ca, sa = mp.cos(theta), mp.sin(theta), mp.cos(alpha), mp.sin(alpha)
    z, o = mpf(0), mpf(1)
    return [[ct, -st, z, a], [st * ca, ct * ca, -sa, -sa * d], [st * sa, ct * sa, ca, ca * d], [z, z, z, o]]


def _mp_tool(tool):
    if tool is None or isinstance(tool, str):
        rows = {None: evaluation.EE_STATIC_DH, "flange": evaluation.EE_STATIC_DH[:1], "hand": evaluation.EE_STATIC_DH[:2]}[tool]
        T = _eye()
        for a, d, al, th in rows:
            T = _mul(T, _mp_dh(a, d, al, th))
        return T
    m = np.asarray(tool, dtype=np.float64)
    T = _eye()
    for a in range(3):
        for b in range(4):
            T[a][b] = mpf(float(m[a, b]))
    return T


def _mp_links(q):
    return [_mp_dh(*(float(v) for v in franka.DH_A_D_ALPHA[j]), q[j]) for j in range(7)]


def _mp_fk(q, tool4):
    T = _eye()
    for D in _mp_links(q):
        T = _mul(T, D)
    return _mul(T, tool4)


def mp_fk(q, tool=None):
    """the tool pose at q (7,) as a 4 x 4 list of mpf"""
    with mp.workdps(DPS):
        return _mp_fk([mpf(float(v)) for v in q], _mp_tool(tool))


def _mp_jacobian(q, tool4, T0):
    """6 x 7: rows 0-2 dp/dq_j, rows 3-5 vee((dR/dq_j) R^T), by central differences of the FK.  FK(q +- h e_j) is the same product of
    ten matrices with row j re-evaluated; the products before and behind row j are shared between the fourteen evaluations"""
    links = _mp_links(q)
    before, behind = [_eye()], [tool4]
    for j in range(6):
        before.append(_mul(before[-1], links[j]))
    for j in range(6, 0, -1):
        behind.append(_mul(links[j], behind[-1]))
    behind.reverse()
    J = [[None] * 7 for _ in range(6)]
    for j in range(7):
        a, d, al = (float(v) for v in franka.DH_A_D_ALPHA[j])
        Tp = _mul(before[j], _mul(_mp_dh(a, d, al, q[j] + H), behind[j]))
        Tm = _mul(before[j], _mul(_mp_dh(a, d, al, q[j] - H), behind[j]))
        dT = [[(Tp[a][b] - Tm[a][b]) / (2 * H) for b in range(4)] for a in range(3)]
        S = [[sum(dT[a][c] * T0[b][c] for c in range(3)) for b in range(3)] for a in range(3)]  # (dR/dq_j) R^T, skew
        for a in range(3):
            J[a][j] = dT[a][3]
        J[3][j] = (S[2][1] - S[1][2]) / 2
        J[4][j] = (S[0][2] - S[2][0]) / 2
        J[5][j] = (S[1][0] - S[0][1]) / 2
    return J


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _mp_error(T0, Tt):
    """e = [p_t - p ; 1/2 sum_k R[:,k] x R_t[:,k]] and the trace of R^T R_t, as include/edmp_hip.h states them"""
    ep = [Tt[a][3] - T0[a][3] for a in range(3)]
    er = [mpf(0)] * 3
    tr = mpf(0)
    for k in range(3):
        c = _cross([T0[a][k] for a in range(3)], [Tt[a][k] for a in range(3)])
        er = [er[a] + c[a] / 2 for a in range(3)]
        tr += sum(T0[a][k] * Tt[a][k] for a in range(3))
    return ep, er, tr


def _mp_residuals(T0, Tt):
    ep, er, tr = _mp_error(T0, Tt)
    return mp.sqrt(sum(v * v for v in ep)), mp.atan2(mp.sqrt(sum(v * v for v in er)), (tr - 1) / 2)


def _mp_step(q, Tt, tool4, lam, max_step, lo, hi):
    T0 = _mp_fk(q, tool4)
    ep, er, _ = _mp_error(T0, Tt)
    e = ep + er
    J = _mp_jacobian(q, tool4, T0)
    A = mp.matrix(6, 6)
    for a in range(6):
        for b in range(6):
            A[a, b] = sum(J[a][j] * J[b][j] for j in range(7)) + (lam * lam if a == b else 0)
    y = mp.lu_solve(A, mp.matrix(e))
    dq = [sum(J[a][j] * y[a] for a in range(6)) for j in range(7)]
    big = max(abs(v) for v in dq)
    scale = max_step / big if big > max_step else mpf(1)
    return [min(max(q[j] + scale * dq[j], lo[j]), hi[j]) for j in range(7)]


_CHAINS = {}  # (target, seed, tool, damping, max_step) -> [q_0, q_1, ...] as lists of mpf


def mp_iterate(target, seed, k, tool=None, damping=I.DAMPING, max_step=I.MAX_STEP):
    """k steps of the iteration from `seed` (7,) towards `target` (4, 4) at 50 digits -> (q_k (7,) f64, (pos, ang) f64): the state and
    its residuals, rounded to f64 at the very end.  A chain is kept per process: asking for k after k - 1 costs one step."""
    target, seed = np.asarray(target, dtype=np.float64), np.asarray(seed, dtype=np.float64)
    tkey = tool if tool is None or isinstance(tool, str) else np.asarray(tool, dtype=np.float64).tobytes()
    key = (target.tobytes(), seed.tobytes(), tkey, float(damping), float(max_step))
    with mp.workdps(DPS):
        lo, hi = ([mpf(float(v)) for v in lim] for lim in franka.joint_limits())
        tool4 = _mp_tool(tool)
        Tt = [[mpf(float(target[a, b])) for b in range(4)] for a in range(4)]
        chain = _CHAINS.setdefault(key, [[mpf(float(v)) for v in seed]])
        while len(chain) <= k:
            chain.append(_mp_step(chain[-1], Tt, tool4, mpf(float(damping)), mpf(float(max_step)), lo, hi))
        q = chain[k]
        pos, ang = _mp_residuals(_mp_fk(q, tool4), Tt)
        return np.array([float(v) for v in q]), (float(pos), float(ang))


# ---- the second f64 formulation -----------------------------------------------------------------------------------------------------


def dls_cholesky(target, seeds, tool=None, iters=I.ITERS, damping=I.DAMPING, max_step=I.MAX_STEP, return_big=False):
    """the iteration for one target (4, 4) and seeds (n, 7) -> q (n, 7) [, the unscaled max |dq| of every iteration (iters, n)]"""
    lo, hi = franka.joint_limits()
    tool4 = I.tool_matrix(tool)
    Rt, pt = np.asarray(target)[:3, :3], np.asarray(target)[:3, 3]
    q = np.array(seeds, dtype=np.float64)
    n = q.shape[0]
    bigs = []
    for _ in range(int(iters)):
        R = np.broadcast_to(np.eye(3), (n, 3, 3))
        o = np.zeros((n, 3))
        z, p = [], []
        for j in range(7):
            a, d, al = franka.DH_A_D_ALPHA[j]
            cq, sq, ca, sa = np.cos(q[:, j]), np.sin(q[:, j]), np.cos(al), np.sin(al)
            o = o + R[:, :, 0] * a + (R[:, :, 2] * ca - R[:, :, 1] * sa) * d  # Rot_x(alpha) then the z offset d
            x, y, zz = R[:, :, 0], R[:, :, 1] * ca + R[:, :, 2] * sa, R[:, :, 2] * ca - R[:, :, 1] * sa
            R = np.stack([x * cq[:, None] + y * sq[:, None], y * cq[:, None] - x * sq[:, None], zz], axis=2)
            z.append(zz)
            p.append(o)
        pe = o + np.einsum("nab,b->na", R, tool4[:3, 3])
        Re = np.einsum("nab,bc->nac", R, tool4[:3, :3])
        e = np.concatenate([pt[None] - pe, 0.5 * sum(np.cross(Re[:, :, k], Rt[None, :, k]) for k in range(3))], axis=1)
        cols = [np.concatenate([np.cross(z[j], pe - p[j]), z[j]], axis=1) for j in range(7)]  # (n, 6) per joint
        A = np.zeros((n, 6, 6))
        for j in reversed(range(7)):
            A = A + cols[j][:, :, None] * cols[j][:, None, :]
        A = A + damping * damping * np.eye(6)
        L = np.zeros((n, 6, 6))
        for a in range(6):
            for b in range(a + 1):
                s = A[:, a, b] - sum(L[:, a, k] * L[:, b, k] for k in range(b))
                L[:, a, b] = np.sqrt(s) if a == b else s / L[:, b, b]
        y = np.zeros((n, 6))
        for a in range(6):
            y[:, a] = (e[:, a] - sum(L[:, a, k] * y[:, k] for k in range(a))) / L[:, a, a]
        for a in reversed(range(6)):
            y[:, a] = (y[:, a] - sum(L[:, k, a] * y[:, k] for k in range(a + 1, 6))) / L[:, a, a]
        dq = np.stack([np.sum(cols[j] * y, axis=1) for j in range(7)], axis=1)
        big = np.max(np.abs(dq), axis=1)
        bigs.append(big)
        scale = np.where(big > max_step, max_step / np.where(big > 0, big, 1.0), 1.0)
        q = np.minimum(np.maximum(q + scale[:, None] * dq, lo), hi)
    return (q, np.stack(bigs)) if return_big else q


# ---- inputs of the settings -----------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def setting_inputs(name):
    """(targets (T, 4, 4), list of T seed arrays): the full 8 x 256 for "default"; for the others the first three target configurations
    posed in that setting's tool frame, with the first 64 seeds of each"""
    if name == "default":
        return I.targets(), I.seeds()
    tool = SETTINGS[name]["tool"]
    tg = np.stack([I.fk(q, tool) for q in I.target_configurations()[:SETTING_TARGETS]])
    tg.setflags(write=False)
    return tg, [I.seeds()[t][:SETTING_SEEDS] for t in range(SETTING_TARGETS)]


def mp_rows(name):
    """[(target index, seed row)] of the rows of setting `name` that are also iterated in mpmath"""
    n = MP_SEEDS_PER_TARGET if name == "default" else SETTING_MP_SEEDS
    return [(t, r) for t in range(len(setting_inputs(name)[1])) for r in range(n)]


@functools.lru_cache(maxsize=None)
def special_seeds():
    """{(target index, name): seed (7,)} for targets 0 and 5: the edges of the limits, the two wrist / shoulder alignments, the
    neighbourhood of the solution and the solution itself"""
    lo, hi = franka.joint_limits()
    out = {}
    for t in SPECIAL_TARGETS:
        base, own = I.seeds()[t][0], I.target_configurations()[t]
        q2, q6 = base.copy(), base.copy()
        q2[1] = 0.0  # axes 1 and 3 in line
        q6[5] = 0.0  # axes 5 and 7 in line
        for name, s in (("all_lo", lo.copy()), ("all_hi", hi.copy()), ("alternating", np.where(np.arange(7) % 2 == 0, lo, hi)), ("q2_zero", q2), ("q6_zero", q6),
                        ("own_plus_1e-3", own + 1e-3), ("own_plus_1e-6", own + 1e-6), ("own", own.copy())):
            assert (s >= lo).all() and (s <= hi).all(), (t, name)
            s.setflags(write=False)
            out[(t, name)] = s
    return out


@functools.lru_cache(maxsize=None)
def restatement(name, k):
    """dls_numpy of every row of setting `name` after k iterations: tuple per target of (q, residuals, valid), read-only"""
    tg, sd = setting_inputs(name)
    out = []
    for t in range(len(sd)):
        res = I.dls_numpy(tg[t], sd[t], iters=k, **SETTINGS[name])
        for a in res:
            a.setflags(write=False)
        out.append(res)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def special_floors():
    """for the special seeds, k = 1, 2, 3: floor_mp, floor_f64 and gate_mp = 100 x max of the two, over the sixteen of them"""
    f_mp, f_64 = {k: 0.0 for k in SPECIAL_KS}, {k: 0.0 for k in SPECIAL_KS}
    for (t, _), s in special_seeds().items():
        tg = I.targets()[t]
        for k in SPECIAL_KS:
            qn = I.dls_numpy(tg, s[None], iters=k)[0][0]
            f_mp[k] = max(f_mp[k], float(np.max(np.abs(qn - mp_iterate(tg, s, k)[0]))))
            f_64[k] = max(f_64[k], float(np.max(np.abs(qn - dls_cholesky(tg, s[None], iters=k)[0]))))
    return dict(floor_mp=f_mp, floor_f64=f_64, gate_mp={k: MARGIN * max(f_mp[k], f_64[k]) for k in SPECIAL_KS})


@functools.lru_cache(maxsize=None)
def floors(name="default"):
    """dict(ks, mp_ks, floor_f64, floor_mp, gate, gate_mp) of a setting (module docstring).  For "default", floor_mp[1] also covers the
    special seeds at k = 1"""
    tg, sd = setting_inputs(name)
    par = SETTINGS[name]
    ks, mp_ks = (FULL_KS, MP_KS) if name == "default" else (SETTING_KS, SETTING_KS)
    f_64 = {k: max(float(np.max(np.abs(restatement(name, k)[t][0] - dls_cholesky(tg[t], sd[t], iters=k, **par)))) for t in range(len(sd))) for k in ks}
    f_mp = {k: max(float(np.max(np.abs(restatement(name, k)[t][0][r] - mp_iterate(tg[t], sd[t][r], k, **par)[0]))) for t, r in mp_rows(name)) for k in mp_ks}
    if name == "default":
        f_mp[1] = max(f_mp[1], special_floors()["floor_mp"][1])
    return dict(ks=ks, mp_ks=mp_ks, floor_f64=f_64, floor_mp=f_mp, gate={k: MARGIN * f_64[k] for k in ks}, gate_mp={k: MARGIN * max(f_mp[k], f_64[k]) for k in mp_ks})


def near_tolerance(name, k, tol_pos=I.TOL_POS, tol_ang=I.TOL_ANG):
    """bool per row (all targets concatenated): a residual of the restatement lies within gate[k] of its tolerance, so that a correct
    kernel may put the row on the other side of the validity rule"""
    g = floors(name)["gate"][k]
    res = np.concatenate([r for _, r, _ in restatement(name, k)])
    return (np.abs(res[:, 0] - tol_pos) <= g) | (np.abs(res[:, 1] - tol_ang) <= g)
