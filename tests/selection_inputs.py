"""Inputs of the reduction tests (test infrastructure, no GPU needed): the rules of the row reductions stated once in plain Python -
sequential loops over Python floats - and the seeded inputs that hold the kernels to them past one element per lane.

argmin_rule is argmin_kernel's contract (csrc/guide.hip; torch.argmin as lib/guide.py:650 uses it), select_rule the contract of
edmp_select_row_dev in include/edmp_hip.h (segment_select, csrc/pick.h): vol_tie = False is the pick among plans
(select_row_kernel), vol_tie = True the pick among IK goals (goal_pick_kernel).

All volumes are level * 2^-12 as f32 with level in 0..7 and every trust region is exact in f64, so no volume lies near a threshold:
with trust = 0.0008 the levels 0..3 (<= 7.33e-4) are inside and 4..7 (>= 9.77e-4) outside of a minimum at level 0; the nearest level is
6.8e-5 away.  Keys are drawn from {0., 1., 2., 3.}: ties are everywhere, in the volumes and in the keys.

tests/test_selection_rules_host.py checks on the CPU that the rules are torch.argmin's / np.argmin's / guide.pick_goal's and that
every family is what it claims to be; tests/test_gpu_reductions.py holds the kernels to the rules on the same inputs."""
import math

import numpy as np

ARGMIN_SIZES = (1, 2, 63, 64, 65, 128, 129, 257, 1025)  # argmin_kernel: one wave, lane = i % 64
PICK_SIZES = (1, 64, 65, 255, 256, 257, 513, 1025)      # segment_select: 256 threads = four waves, thread = b % 256
TRUSTS = (0.0, 0.0008, 1.0, math.inf)
UNIT = 2.0 ** -12
LEVELS, INSIDE = 8, 4  # levels 0..INSIDE-1 lie within 0.0008 of level 0
KEYS = (0.0, 1.0, 2.0, 3.0)
ARGMIN_LANES, PICK_THREADS, WAVE = 64, 256, 64
# tie pairs (i, j), i < j, where j sits in a lower lane / thread than i - the first index has to win against the order of the lanes
ARGMIN_PAIR = (70, 129)     # lanes 6 and 1
PICK_PAIR = (200, 257)      # threads 200 and 1
PICK_WAVE_PAIR = (65, 259)  # threads 65 (wave 1) and 3 (wave 0)


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
def argmin_rule(v):
    """first index of the minimum; NaN beats every number; among NaNs and among equal numbers (-0.0 == 0.0) the lower index wins"""
    best = None
    for i, x in enumerate(v):
        x = float(x)
        if best is None:
            best, bx = i, x
            continue
        if bx != bx:        # a NaN holds the place: nothing later beats it
            continue
        if x != x or x < bx:
            best, bx = i, x
    return best


def select_rule(vol_f32, key_f64, trust, vol_tie):
    """edmp_select_row_dev's contract: m = argmin_rule(vol); a NaN vol[m] keeps m; the candidates are the rows with
    float(v_b) < float(v_m) + trust (f64: -inf + inf is NaN and admits nothing); among the candidates with a finite key the smallest
    key; on equal keys vol_tie = False takes the lower index, vol_tie = True the smaller volume, then the lower index; m when no
    candidate has a finite key"""
    m = argmin_rule(vol_f32)
    vm = float(vol_f32[m])
    if vm != vm:
        return m
    bound = vm + float(trust)
    pick = None
    for b in range(len(vol_f32)):
        vb, kb = float(vol_f32[b]), float(key_f64[b])
        if not vb < bound or not math.isfinite(kb):
            continue
        if pick is None or kb < pk or (vol_tie and kb == pk and vb < pv):
            pick, pk, pv = b, kb, vb
    return m if pick is None else pick


# ---- the value families ---------------------------------------------------------------------------------------------------------------
def _seed(tag, n):
    return (sum(ord(c) * (k + 1) for k, c in enumerate(tag)) * 7919 + 31 * n) % (2 ** 31)


def _plain(rs, n, lo=0):
    """(a): quantised volumes (levels lo..7) and keys from KEYS"""
    vol = (rs.randint(lo, LEVELS, n) * UNIT).astype(np.float32)
    key = np.asarray(KEYS)[rs.randint(0, len(KEYS), n)].astype(np.float64)
    return vol, key


def _some(rs, n, share):
    """a seeded subset of about `share` of the n places - never empty, never everything once n >= 2"""
    hit = rs.uniform(size=n) < share
    if n >= 2:
        if not hit.any():
            hit[rs.randint(n)] = True
        if hit.all():
            hit[rs.randint(n)] = False
    return hit


def families(n):
    """{name: (vol (n,) f32, key (n,) f64)} - the families (a) .. (e) at size n, seeded by (name, n)"""
    out = {}
    out["a_plain"] = _plain(np.random.RandomState(_seed("a", n)), n)
    # (b) about 2 % NaN volumes
    rs = np.random.RandomState(_seed("b", n))
    vol, key = _plain(rs, n)
    vol[_some(rs, n, 0.02)] = np.nan
    out["b_nan_volumes"] = (vol, key)
    # (c) NaN, +inf and -inf keys sprinkled in; one variant without a finite key
    rs = np.random.RandomState(_seed("c", n))
    vol, key = _plain(rs, n)
    for bad in (np.nan, np.inf, -np.inf):
        key[_some(rs, n, 0.08)] = bad
    out["c_odd_keys"] = (vol, key)
    rs = np.random.RandomState(_seed("c0", n))
    vol, _ = _plain(rs, n)
    out["c_no_finite_key"] = (vol, np.asarray([np.nan, np.inf, -np.inf])[rs.randint(0, 3, n)])
    # (d) volumes all +inf; one -inf among finite values; a mix of -0.0 and 0.0
    rs = np.random.RandomState(_seed("d", n))
    _, key = _plain(rs, n)
    out["d_all_inf"] = (np.full(n, np.inf, dtype=np.float32), key)
    vol, key = _plain(rs, n)
    vol[(2 * n) // 3] = -np.inf
    out["d_one_neg_inf"] = (vol, key)
    _, key = _plain(rs, n)
    out["d_signed_zeros"] = (np.where(rs.randint(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32), key)
    # (e) a unique minimum at n - 1, 63, 64, 255, 256 (where the size holds that index)
    for p in sorted({q for q in (n - 1, 63, 64, 255, 256) if q < n}):
        vol, key = _plain(np.random.RandomState(_seed(f"e{p}", n)), n, lo=1)
        vol[p] = 0.0
        out[f"e_min_at_{p}"] = (vol, key)
    return out


def _placed(n, pair, seed):
    """levels 1..3 and keys 1..3 everywhere, level 0 and key 0 at both members of `pair`: they tie for the minimum volume and for the
    smallest key inside every trust region"""
    rs = np.random.RandomState(seed)
    vol = (rs.randint(1, INSIDE, n) * UNIT).astype(np.float32)
    key = np.asarray(KEYS[1:])[rs.randint(0, 3, n)].astype(np.float64)
    vol[list(pair)] = 0.0
    key[list(pair)] = 0.0
    return vol, key


def _later_is_smaller(n, pair, seed):
    """equal minimal keys at both members of `pair`, the LATER one with the smaller volume (level 1 against 2), both inside the trust
    region of a level-0 row with the largest key: vol_tie = False has to take the first index, vol_tie = True the later"""
    rs = np.random.RandomState(seed)
    vol = (rs.randint(2, INSIDE, n) * UNIT).astype(np.float32)
    key = np.asarray(KEYS[1:])[rs.randint(0, 3, n)].astype(np.float64)
    i, j = pair
    vol[i], vol[j] = 2 * UNIT, 1 * UNIT
    key[i] = key[j] = 0.0
    vol[0], key[0] = 0.0, 3.0
    return vol, key


def argmin_inputs():
    """[(name, n, vol (n,) f32)]: every family's volumes at every arg-min size, and the placed pair"""
    out = [(f"{name}/n={n}", n, vol) for n in ARGMIN_SIZES for name, (vol, _) in families(n).items()]
    for n in (129 + 1, 257, 1025):
        out.append((f"placed_{ARGMIN_PAIR}/n={n}", n, _placed(n, ARGMIN_PAIR, 900 + n)[0]))
    return out


def pick_inputs():
    """[(name, n, vol (n,) f32, key (n,) f64)]: every family at every pick size, the placed pairs, and the pairs whose later member
    has the smaller volume"""
    out = [(f"{name}/n={n}", n, vol, key) for n in PICK_SIZES for name, (vol, key) in families(n).items()]
    for pair in (PICK_PAIR, PICK_WAVE_PAIR):
        for n in (pair[1] + 1, 513, 1025):
            out.append((f"placed_{pair}/n={n}", n, *_placed(n, pair, 1000 + n + pair[0])))
            out.append((f"later_is_smaller_{pair}/n={n}", n, *_later_is_smaller(n, pair, 2000 + n + pair[0])))
    return out


def packed(inputs):
    """all inputs of argmin_inputs() / pick_inputs() behind one another, for ONE upload: (offsets, vol (sum n,) f32, key (sum n,) f64
    or None); input k is [offsets[k], offsets[k] + n_k)"""
    off = np.concatenate([[0], np.cumsum([c[1] for c in inputs])]).astype(np.int64)
    vol = np.ascontiguousarray(np.concatenate([c[2] for c in inputs]).astype(np.float32))
    key = np.ascontiguousarray(np.concatenate([c[3] for c in inputs]).astype(np.float64)) if len(inputs[0]) > 3 else None
    return off, vol, key
