"""Inputs and CPU reference of the self-collision tests (test infrastructure).

Inputs: RandomState(7), 96 rows; each row a straight joint-space line between two configurations uniform in the joint limits, N = 50,
plus 0.02 * randn.  With the default pair mask (franka.self_collision_pairs()) and substeps = 4: 24 colliding and 72 free rows.

Reference: oracle.success_oracle.link_box_poses_batch + obb_overlap_batch (NumPy; they share no code with csrc/selfcol.hip).  The key of a
row is its first colliding configuration, then the first masked pair in row-major order that overlaps there.

Condition: the decision distance of every (row, configuration, masked pair) - how far the pair is from the boundary of the separating-axis
decision, in metres along the deciding axis - is >= MIN_DECISION (1e-9 m, the success tests' own margin).  `reference` asserts it for
every row it is given; no row is left out.
"""
import functools

import numpy as np

from edmp_amd import franka
from oracle import success_oracle as SO

SEED, ROWS, N = 7, 96, 50
MIN_DECISION = 1e-9


def rows(n=ROWS, N=N, seed=SEED):
    """(n, 7, N) f64: the recipe of the module docstring"""
    rs = np.random.RandomState(seed)
    lo, hi = franka.joint_limits()
    a, b = rs.uniform(lo, hi, (n, 7)), rs.uniform(lo, hi, (n, 7))
    t = np.linspace(0, 1, N)
    X = a[:, :, None] * (1 - t) + b[:, :, None] * t
    return np.ascontiguousarray(X + 0.02 * rs.standard_normal((n, 7, N)))


def configurations(X, substeps):
    """(n, 7, N) -> (n, nc, 7): the success check's configurations (oracle.success_oracle.success_rows' own expression)"""
    X = np.asarray(X, dtype=np.float64)
    n, _, Nw = X.shape
    S = int(substeps)
    Q = np.zeros((n, (Nw - 1) * S + 1, 7))
    for i in range(Nw):
        for s in range(S if i < Nw - 1 else 1):
            f = s / S
            Q[:, i * S + s] = X[:, :, i] if s == 0 else (1 - f) * X[:, :, i] + f * X[:, :, i + 1]
    return Q


def sat_margin(Ra, ca, ha, Rb, cb, hb):
    """the largest signed gap over the 15 candidate axes, each divided by its axis length (cross axes shorter than 1e-6 are left to the
    face axes): > 0 separated by that much along the deciding axis, < 0 overlapping.  Written apart from the oracle's test and from the
    kernel: it measures how far a decision is from flipping, it does not decide."""
    R = np.einsum("...ki,...kj->...ij", Ra, Rb)
    t = np.einsum("...ki,...k->...i", Ra, cb - ca)
    A = np.abs(R)
    gaps = []
    for i in range(3):
        gaps.append(np.abs(t[..., i]) - (ha[i] + A[..., i, :] @ hb))
    for j in range(3):
        gaps.append(np.abs(np.einsum("...i,...i->...", t, R[..., :, j])) - (np.einsum("i,...i->...", ha, A[..., :, j]) + hb[j]))
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            ra = ha[i1] * A[..., i2, j] + ha[i2] * A[..., i1, j]
            rb = hb[j1] * A[..., i, j2] + hb[j2] * A[..., i, j1]
            ln = np.sqrt(np.maximum(1.0 - R[..., i, j] ** 2, 0.0))
            g = (np.abs(t[..., i2] * R[..., i1, j] - t[..., i1] * R[..., i2, j]) - (ra + rb)) / np.maximum(ln, 1e-6)
            gaps.append(np.where(ln >= 1e-6, g, -np.inf))
    return np.max(np.stack(gaps), axis=0)


def reference(X, substeps=4, mask=None):
    """-> dict(first (n,) int32, pair (n, 2) int32 with -1 rows, free (n,) bool, decision (n,) f64 = the row's smallest decision distance,
    inf without a masked pair).  Asserts the module's condition on every row."""
    X = np.asarray(X, dtype=np.float64)
    mask = franka.self_collision_pairs() if mask is None else np.asarray(mask)
    n = X.shape[0]
    S = int(substeps)
    Q = configurations(X, S)
    nc = Q.shape[1]
    he = franka.link_half_extents().astype(np.float64)
    Rl, cl = SO.link_box_poses_batch(Q.reshape(-1, 7))
    key = np.full(n * nc, np.iinfo(np.int64).max, dtype=np.int64)
    decision = np.full(n * nc, np.inf)
    cidx = np.tile(np.arange(nc, dtype=np.int64), n)
    for a in range(9):
        for b in range(a + 1, 9):
            if not mask[a][b]:
                continue
            hit = SO.obb_overlap_batch(Rl[:, a], cl[:, a], he[a], Rl[:, b], cl[:, b], he[b])
            key = np.where(hit, np.minimum(key, cidx * 81 + a * 9 + b), key)
            decision = np.minimum(decision, np.abs(sat_margin(Rl[:, a], cl[:, a], he[a], Rl[:, b], cl[:, b], he[b])))
    key = key.reshape(n, nc).min(axis=1)
    decision = decision.reshape(n, nc).min(axis=1)
    assert np.all(decision >= MIN_DECISION), ("rows too close to the separating-axis decision boundary", np.nonzero(decision < MIN_DECISION)[0], decision.min())
    free = key == np.iinfo(np.int64).max
    k = np.where(free, 0, key)
    first = np.where(free, -1, (k // 81) // S).astype(np.int32)
    pair = np.where(free[:, None], -1, np.stack([(k % 81) // 9, k % 9], axis=1)).astype(np.int32)
    return dict(first=first, pair=pair, free=free, decision=decision)


@functools.lru_cache(maxsize=None)
def _cached(substeps):
    X = rows()
    ref = reference(X, substeps)
    for v in ref.values():
        v.setflags(write=False)
    X.setflags(write=False)
    return X, ref


def rows_and_reference(substeps=4):
    """the 96 rows and their reference under the default mask, computed once per process and read-only"""
    return _cached(int(substeps))
