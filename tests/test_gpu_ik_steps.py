"""GPU: the IK kernel (csrc/ik.hip: edmp_ik_solve_dev, edmp_ik_compact_dev) held to independent references step by step.

tests/test_gpu_ik.py checks outcomes: a returned goal reproduces its target.  Damped least squares converges with a wrong lever arm, with
lambda for lambda^2, with an L2 step norm or without a clamp - to fewer goals.  Here the ITERATION is compared, per seed, after 1 .. 16
steps, where two correct f64 formulations still agree to 1e-10 and each of those mistakes has moved q by >= 3e-5 rad:

* against tests/ik_inputs.dls_numpy on every row, at gate[k] = 100 x the distance between two f64 formulations on the same rows;
* against tests/ik_reference.mp_iterate (mpmath, 50 digits, the Jacobian obtained by differentiating the FK) on subsets, at
  gate_mp[k] = 100 x max(floor_mp[k], floor_f64[k]).

Floors and gates are computed at test time on the CPU (tests/ik_reference.floors; tests/test_ik_reference_host.py holds them and shows
that every mutant of dls_numpy lies beyond them).  Further: every reported residual, the boundary of the validity rule, the compaction
kernel alone past its 256-row chunk, and the block table over many small blocks.  The measured maxima, floors and gates go to
profiles/ik_parity.json."""
import json
import os

import numpy as np
import pytest

from tests import ik_inputs as I
from tests import ik_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = ("full_set", "mpmath_subset", "settings", "special_seeds", "many_small_blocks")


@pytest.fixture(scope="module")
def parity():
    """what the tests measured; written to profiles/ik_parity.json once every section is in"""
    rec = {}
    yield rec
    if all(s in rec for s in SECTIONS) and len(rec["settings"]) == len(R.SETTINGS) - 1:
        import torch

        ratios = [v for s in rec.values() for v in _ratios(s)]
        out = dict(test="tests/test_gpu_ik_steps.py", device=torch.cuda.get_device_name(0),
                   measure="max |q_gpu - q_ref| [rad] and max |residual_gpu - residual_ref| [m, rad] per iteration count k; floor_f64 = max |dls_numpy - "
                           "dls_cholesky|, floor_mp = max |dls_numpy - mpmath|, gate = 100 floor_f64, gate_mp = 100 max(floor_mp, floor_f64) (tests/ik_reference.py)",
                   largest_measured_over_gate=max(ratios), **rec)
        with open(os.path.join(ROOT, "profiles", "ik_parity.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def _ratios(section):
    if isinstance(section, dict):
        if "over_gate" in section:
            yield section["over_gate"]
        for v in section.values():
            yield from _ratios(v)


def _floors_record(f):
    return {key: {str(k): v for k, v in f[key].items()} for key in ("floor_f64", "floor_mp", "gate", "gate_mp")}


def _solve(targets, seeds, **kw):
    from edmp_amd import ik

    return ik.solve(DEV, targets, seeds, return_all=True, **kw)


def _against_restatement(name, k, out):
    """(max |q - dls_numpy|, max |residuals - dls_numpy's|, rows whose `valid` differs) of one solve of setting `name` at k iterations"""
    ref = R.restatement(name, k)
    q, res, valid = (np.concatenate([r[i] for r in ref]) for i in range(3))
    assert out["q"].shape == q.shape and np.isfinite(out["q"]).all() and np.isfinite(out["residuals"]).all()
    return float(np.max(np.abs(out["q"] - q))), float(np.max(np.abs(out["residuals"] - res))), np.flatnonzero(out["valid"] != valid)


def _against_mpmath(name, k, out, rows):
    tg, sd = R.setting_inputs(name)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sd])])
    dq = dr = 0.0
    for t, r in rows:
        q, (pos, ang) = R.mp_iterate(tg[t], sd[t][r], k, **R.SETTINGS[name])
        dq = max(dq, float(np.max(np.abs(out["q"][off[t] + r] - q))))
        dr = max(dr, abs(out["residuals"][off[t] + r, 0] - pos), abs(out["residuals"][off[t] + r, 1] - ang))
    return dq, dr


@pytest.fixture(scope="module")
def by_k():
    """the 8 x 256 seeds at the defaults after k = 1, 2, 4, 8, 16 iterations, each solved once"""
    return {k: _solve(I.targets(), I.seeds(), iters=k) for k in R.FULL_KS}


def test_a_full_set_against_the_restatement(by_k, parity):
    """3a. all 2048 rows at k = 1 .. 16: q within gate[k] of dls_numpy on EVERY row, both residuals within gate[k] absolute, `valid` equal
    on every row that does not sit within gate[k] of a tolerance (at most 2 such rows: test_ik_reference_host, 2e)"""
    f = R.floors("default")
    rec, failed = {}, []
    for k in R.FULL_KS:
        dq, dr, differ = _against_restatement("default", k, by_k[k])
        near = np.flatnonzero(R.near_tolerance("default", k))
        gate = f["gate"][k]
        rec[str(k)] = dict(max_abs_dq=dq, max_abs_dresidual=dr, gate=gate, over_gate=max(dq, dr) / gate, valid_rows=int(by_k[k]["valid"].sum()),
                           rows_left_out_of_valid=int(near.size))
        print(f"[ik steps] k={k}: max |dq| {dq:.3e}, max |dres| {dr:.3e}, gate {gate:.3e} (floor_f64 {f['floor_f64'][k]:.3e}); valid {int(by_k[k]['valid'].sum())}, "
              f"valid differs on rows {differ.tolist()}, rows at a tolerance {near.tolist()}")
        if not (dq <= gate and dr <= gate and near.size <= 2 and np.isin(differ, near).all()):
            failed.append(k)
    parity["full_set"] = dict(rows=2048, per_k=rec, **_floors_record(f))
    assert not failed, (failed, rec)
    assert by_k[16]["valid"].sum() >= 8  # the validity rule is exercised on both sides at 16 iterations


def test_b_subset_against_mpmath(by_k, parity):
    """3b. the first 8 seeds of each target against the 50-digit iteration whose Jacobian is the differentiated FK, k = 1, 2, 4"""
    f = R.floors("default")
    rec = {}
    for k in R.MP_KS:
        dq, dr = _against_mpmath("default", k, by_k[k], R.mp_rows("default"))
        gate = f["gate_mp"][k]
        rec[str(k)] = dict(max_abs_dq=dq, max_abs_dresidual=dr, gate_mp=gate, over_gate=max(dq, dr) / gate)
        print(f"[ik steps] mpmath k={k}: max |dq| {dq:.3e}, max |dres| {dr:.3e}, gate_mp {gate:.3e} (floor_mp {f['floor_mp'][k]:.3e})")
    parity["mpmath_subset"] = dict(rows=len(R.mp_rows("default")), per_k=rec)
    for k in R.MP_KS:
        assert rec[str(k)]["over_gate"] <= 1.0, rec


@pytest.mark.parametrize("name", [n for n in R.SETTINGS if n != "default"])
def test_c_other_parameters_and_frames(name, parity):
    """3c. damping 0.1 / max_step 0.05 (every step scaled), damping 1e-3 / max_step 2 (many unscaled), the flange frame and a rotated and
    offset custom frame (where a lever arm that forgets the tool offset shows only against the differentiated Jacobian): 3 targets x 64
    seeds at k = 1 and 4 against dls_numpy, 4 seeds each against mpmath, with that setting's own floors and gates"""
    f = R.floors(name)
    tg, sd = R.setting_inputs(name)
    rec = {}
    for k in R.SETTING_KS:
        out = _solve(tg, sd, iters=k, **R.SETTINGS[name])
        dq, dr, differ = _against_restatement(name, k, out)
        mq, mr = _against_mpmath(name, k, out, R.mp_rows(name))
        near = np.flatnonzero(R.near_tolerance(name, k))
        rec[str(k)] = dict(max_abs_dq=dq, max_abs_dresidual=dr, gate=f["gate"][k], over_gate=max(dq, dr) / f["gate"][k],
                           mpmath=dict(max_abs_dq=mq, max_abs_dresidual=mr, gate_mp=f["gate_mp"][k], over_gate=max(mq, mr) / f["gate_mp"][k]))
        print(f"[ik steps] {name} k={k}: restatement max |dq| {dq:.3e} |dres| {dr:.3e} gate {f['gate'][k]:.3e}; mpmath max |dq| {mq:.3e} |dres| {mr:.3e} "
              f"gate_mp {f['gate_mp'][k]:.3e}; valid differs on {differ.tolist()}, at a tolerance {near.tolist()}")
        assert near.size <= 2 and np.isin(differ, near).all()
    parity.setdefault("settings", {})[name] = dict(rows=192, mpmath_rows=12, damping=R.SETTINGS[name]["damping"], max_step=R.SETTINGS[name]["max_step"], per_k=rec,
                                                   **_floors_record(f))
    for k in R.SETTING_KS:
        assert rec[str(k)]["over_gate"] <= 1.0 and rec[str(k)]["mpmath"]["over_gate"] <= 1.0, rec


def test_d_special_seeds_against_mpmath(parity):
    """3d. for targets 0 and 5: all joints at lo, at hi, alternating; q2 = 0 and q6 = 0 (two axes in line); the solution + 1e-3, + 1e-6,
    and the solution itself - k = 1, 2, 3 against mpmath, gate 100 x max(floor_mp, floor_f64) over these sixteen seeds"""
    sp = R.special_floors()
    keys = list(R.special_seeds())
    rec, worst = {}, {}
    for k in R.SPECIAL_KS:
        out = {t: _solve(I.targets()[t:t + 1], [np.stack([R.special_seeds()[key] for key in keys if key[0] == t])], iters=k) for t in R.SPECIAL_TARGETS}
        for t in R.SPECIAL_TARGETS:
            for i, key in enumerate(kk for kk in keys if kk[0] == t):
                q, (pos, ang) = R.mp_iterate(I.targets()[t], R.special_seeds()[key], k)
                d = max(float(np.max(np.abs(out[t]["q"][i] - q))), abs(out[t]["residuals"][i, 0] - pos), abs(out[t]["residuals"][i, 1] - ang))
                worst[(k, key)] = d
        m = max(v for (kk, _), v in worst.items() if kk == k)
        rec[str(k)] = dict(max_abs_d=m, gate_mp=sp["gate_mp"][k], floor_mp=sp["floor_mp"][k], floor_f64=sp["floor_f64"][k], over_gate=m / sp["gate_mp"][k])
        print(f"[ik steps] special seeds k={k}: max |d| {m:.3e}, gate_mp {sp['gate_mp'][k]:.3e}; worst seed {max((v, key) for (kk, key), v in worst.items() if kk == k)}")
    parity["special_seeds"] = dict(rows=len(keys), per_k=rec)
    for k in R.SPECIAL_KS:
        assert rec[str(k)]["over_gate"] <= 1.0, rec


@pytest.fixture(scope="module")
def default_run():
    return _solve(I.targets(), I.seeds())


def test_e_every_residual_is_the_host_fk_s(default_run):
    """3e. at the default 64 iterations, `residuals` of all 2048 rows - valid or not - against the f64 FK of the returned q"""
    q, res = default_run["q"], default_run["residuals"]
    worst = [0.0, 0.0]
    for t in range(8):
        for r in range(256 * t, 256 * (t + 1)):
            pos, ang = I.pose_error(I.fk(q[r]), I.targets()[t])
            worst = [max(worst[0], abs(pos - res[r, 0])), max(worst[1], abs(ang - res[r, 1]))]
    print(f"[ik steps] residuals against the host FK on 2048 rows ({int(default_run['valid'].sum())} valid): max |dpos| {worst[0]:.3e} m, max |dang| {worst[1]:.3e} rad")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-9, worst
    assert (~default_run["valid"]).sum() >= 256  # invalid rows are in the comparison


def test_f_the_boundary_of_the_validity_rule(default_run):
    """3f. tolerances do not enter the iteration: with tol_pos (then tol_ang) set to a valid row's own residual and to the next f64 below
    it, q and residuals stay bit-identical, `valid` is the elementwise <= rule, and that row flips; with both 0, valid = (res == 0)"""
    q, res, valid = default_run["q"], default_run["residuals"], default_run["valid"]
    assert np.array_equal(valid, (res[:, 0] <= I.TOL_POS) & (res[:, 1] <= I.TOL_ANG))
    for col, name, other in ((0, "tol_pos", I.TOL_ANG), (1, "tol_ang", I.TOL_POS)):
        rows = np.flatnonzero(valid)
        r = rows[np.argmax(res[rows, col])]
        at = float(res[r, col])
        below = float(np.nextafter(at, 0.0))
        assert 0.0 < below < at
        flags = {}
        for tol in (at, below):
            out = _solve(I.targets(), I.seeds(), **{name: tol})
            assert np.array_equal(out["q"], q) and np.array_equal(out["residuals"], res)
            tols = (tol, other) if col == 0 else (other, tol)
            assert np.array_equal(out["valid"], (res[:, 0] <= tols[0]) & (res[:, 1] <= tols[1]))
            assert np.array_equal(out["counts"], out["valid"].reshape(8, 256).sum(axis=1))
            flags[tol] = bool(out["valid"][r])
        assert flags[at] and not flags[below], (name, r, at)
    out = _solve(I.targets(), I.seeds(), tol_pos=0.0, tol_ang=0.0)
    assert np.array_equal(out["q"], q) and np.array_equal(out["residuals"], res)
    assert np.array_equal(out["valid"], (res == 0).all(axis=1)) and np.array_equal(out["counts"], out["valid"].reshape(8, 256).sum(axis=1))


COMPACT_GROUPS = [(1,), (63, 64), (257, 1, 513), (512, 256, 1025), (65, 255, 256, 511), (1025, 513, 257, 64, 1)]
PATTERNS = ("all", "none", "first", "last", "row255", "row256", "alternating", "bernoulli_0.1", "bernoulli_0.9", "gap")


def _flags(pattern, n, t, T, rs):
    v = np.zeros(n, dtype=np.int32)
    if pattern == "all":
        v[:] = 1
    elif pattern == "first":
        v[0] = 1
    elif pattern == "last":
        v[-1] = 1
    elif pattern in ("row255", "row256"):  # the last row of the first chunk and the first of the second; a shorter target has none
        r = int(pattern[3:])
        if r < n:
            v[r] = 1
    elif pattern == "alternating":
        v[(t % 2)::2] = 1
    elif pattern.startswith("bernoulli"):
        v[:] = rs.uniform(size=n) < float(pattern.split("_")[1])
    elif pattern == "gap":  # a target without a valid row between two that have some (the inner targets of the group)
        if t in (0, T - 1):
            v[:] = rs.uniform(size=n) < 0.5
            v[n // 2] = 1
    return v


@pytest.mark.parametrize("group", COMPACT_GROUPS)
def test_g_compaction_alone(group):
    """3g. edmp_ik_compact_dev on synthetic inputs, q[r, j] = 8 r + j, goals prefilled with -7: targets of 1 .. 1025 rows around the
    kernel's 256-row chunk, ten flag patterns: counts are the per-target sums, goals[:total] = q[valid] bit for bit, goals[total:] is
    untouched, and a second call gives the same.  Flags are 0 / 1 (the header defines no other value)"""
    import torch

    from edmp_amd import _capi
    from edmp_amd.runtime import get_context, ptr

    ctx = get_context(DEV)
    T, n = len(group), int(sum(group))
    off = np.concatenate([[0], np.cumsum(group)])
    qh = 8.0 * np.arange(n)[:, None] + np.arange(7)[None, :]
    q = torch.from_numpy(qh).to(DEV)
    cn = np.asarray(group, dtype=np.int32)
    rs = np.random.RandomState(1000 + n)
    for pattern in PATTERNS:
        vh = np.concatenate([_flags(pattern, g, t, T, rs) for t, g in enumerate(group)]).astype(np.int32)
        assert set(np.unique(vh)) <= {0, 1} and vh.shape == (n,)
        valid = torch.from_numpy(vh).to(DEV)
        expect = qh[vh.astype(bool)]
        for _ in range(2):
            goals = torch.full((n, 7), -7.0, dtype=torch.float64, device=DEV)
            counts = np.full(T, -7, dtype=np.int32)
            torch.cuda.synchronize()
            assert ctx.lib.edmp_ik_compact_dev(ctx.h, ptr(q), ptr(valid), T, _capi.as_pi32(cn), ptr(goals), _capi.as_pi32(counts)) == 0
            gh = goals.cpu().numpy()
            assert np.array_equal(counts, [vh[off[t]:off[t + 1]].sum() for t in range(T)]), (pattern, counts)
            total = int(counts.sum())
            assert total == expect.shape[0] and np.array_equal(gh[:total], expect), pattern
            assert (gh[total:] == -7.0).all(), pattern
        assert np.array_equal(q.cpu().numpy(), qh) and np.array_equal(valid.cpu().numpy(), vh)
    if T >= 3:  # the conditions the patterns are there for
        gap = [_flags("gap", g, t, T, np.random.RandomState(0)).sum() for t, g in enumerate(group)]
        assert gap[0] > 0 and gap[-1] > 0 and not any(gap[1:-1])


def test_h_past_one_chunk_end_to_end():
    """3h. 257 and 513 seeds for targets 0 and 1 (the compaction's chunk loop runs 2 and 3 times with a carried base): goals are the valid
    rows in seed order, and the first 256 rows of each target are bit-identical to the 256-seed run of the same leading seeds"""
    from edmp_amd import franka

    lo, hi = franka.joint_limits()
    rs = np.random.RandomState(77)
    sd = [np.clip(rs.uniform(lo, hi, (n, 7)), lo, hi) for n in (257, 513)]
    a = _solve(I.targets()[:2], sd)
    b = _solve(I.targets()[:2], [s[:256] for s in sd])
    assert np.array_equal(a["n_seeds"], [257, 513]) and a["q"].shape == (770, 7)
    for t, seg, lead in ((0, slice(0, 257), slice(0, 256)), (1, slice(257, 770), slice(257, 513))):
        v = a["valid"][seg]
        assert a["counts"][t] == v.sum() and np.array_equal(a["goals"][t], a["q"][seg][v])
        assert v[:256].sum() >= 8 and a["counts"][t] >= 8
        for g in a["goals"][t][:4]:
            I.check_goal(g, I.targets()[t])
        one = slice(256 * t, 256 * (t + 1))
        for key in ("q", "residuals", "valid"):
            assert np.array_equal(a[key][lead], b[key][one]), (t, key)
        assert np.array_equal(a["goals"][t][:b["counts"][t]], b["goals"][t])
    assert a["valid"][256] == (a["counts"][0] - b["counts"][0] == 1)  # row 256, the second chunk of target 0, is counted iff it is valid


def test_i_many_small_blocks(parity):
    """3i. 67 targets (the 8 poses cycled) of 1 .. 3 seeds each, 4 iterations: one block per target, so the block table's target index
    and first row are all that tells the blocks apart.  Every row within gate[4] of dls_numpy, ten of them bit-identical to the same
    (target, seed) solved alone"""
    T = 67
    which = [t % 8 for t in range(T)]
    sd = [I.seeds()[which[t]][t:t + 1 + t % 3] for t in range(T)]  # rows t .. t + (t mod 3) of that pose's seeds: distinct per target
    out = _solve(I.targets()[which], sd, iters=4)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sd])])
    assert out["q"].shape == (off[-1], 7) and off[-1] == 133
    gate = R.floors("default")["gate"][4]
    worst = 0.0
    for t in range(T):
        q, res, valid = I.dls_numpy(I.targets()[which[t]], sd[t], iters=4)
        worst = max(worst, float(np.max(np.abs(out["q"][off[t]:off[t + 1]] - q))), float(np.max(np.abs(out["residuals"][off[t]:off[t + 1]] - res))))
        assert (np.abs(res - [I.TOL_POS, I.TOL_ANG]) > gate).all()  # a condition on the inputs: no row at a tolerance
        assert np.array_equal(out["valid"][off[t]:off[t + 1]], valid)
    print(f"[ik steps] 67 small blocks, k=4: max |d| {worst:.3e}, gate {gate:.3e}")
    parity["many_small_blocks"] = dict(rows=int(off[-1]), k=4, max_abs_d=worst, gate=gate, over_gate=worst / gate)
    assert worst <= gate
    for t in (0, 1, 7, 8, 9, 31, 32, 33, 65, 66):
        r = len(sd[t]) - 1
        one = _solve(I.targets()[which[t]][None], [sd[t][r:r + 1]], iters=4)
        assert np.array_equal(one["q"][0], out["q"][off[t] + r]) and np.array_equal(one["residuals"][0], out["residuals"][off[t] + r]), t
