"""Host side of the step-by-step IK tests (no GPU): the references of tests/ik_reference.py are held against each other, the gates the GPU
tests (tests/test_gpu_ik_steps.py) apply are derived from them here, and every deliberate mistake of ik_inputs.dls_numpy(variant=...) is
shown to lie far above those gates.  Nothing in this file runs csrc/ik.hip."""
import numpy as np
import pytest

from tests import ik_inputs as I
from tests import ik_reference as R

# what a correct f64 statement of ONE step may differ by from the 50-digit one: 2^-53 per operation, a few hundred operations, and a
# solve whose condition number is at most |J|^2 / lambda^2 ~ 1e4 - 1e5 at the default damping.  Later steps inherit the earlier error
# through a map that is not contractive far from the solution (a factor of a few per step), which the bound's second factor covers.
PIN_BOUND = 2.0 ** -53 * 300 * 1e5 * 30  # = 1e-7: 300 times below the smallest mutant's 3e-5, so a pinned restatement is not a mutant
MOVED = 1e-6


def test_the_mpmath_fk_is_the_f64_fk_in_every_tool_frame():
    """the two FKs share franka.DH_A_D_ALPHA and evaluation.EE_STATIC_DH and nothing else (one is evaluation._dh in f64)"""
    for tool in (None, "flange", "hand", R.custom_tool()):
        for q in I.target_configurations()[:3]:
            T = np.array([[float(v) for v in row] for row in R.mp_fk(q, tool)])
            assert np.max(np.abs(T - I.fk(q, tool))) < 1e-15


def test_the_differentiated_jacobian_sees_the_tool_offset_and_the_frame():
    """at a configuration away from the solution, the mpmath step equals the restatement's and differs from each mutant that touches the
    Jacobian or the error - in the custom frame too, where the lever arm carries the tool's offset"""
    for name in ("default", "custom"):
        par = R.SETTINGS[name]
        tg, sd = R.setting_inputs(name)
        q_mp = R.mp_iterate(tg[0], sd[0][0], 1, **par)[0]
        assert np.max(np.abs(q_mp - I.dls_numpy(tg[0], sd[0][:1], iters=1, **par)[0][0])) < PIN_BOUND
        for v in ("lever", "lambda", "error_sign", "body_frame_error"):
            assert np.max(np.abs(q_mp - I.dls_numpy(tg[0], sd[0][:1], iters=1, variant=v, **par)[0][0])) > 1e-5, (name, v)


def test_a_the_restatement_is_pinned_to_mpmath():
    """2a. dls_numpy against mp_iterate on the first 8 seeds of each of the 8 targets at k = 1, 2, 4 and on the special seeds at k = 1:
    q and both residuals"""
    f = R.floors("default")
    print("floor_mp (max |dls_numpy - mpmath| over 64 seeds, k = 1 with the 16 special seeds):", f["floor_mp"])
    assert set(f["floor_mp"]) == {1, 2, 4}
    for k in R.MP_KS:
        assert 0 < f["floor_mp"][k] < PIN_BOUND, (k, f["floor_mp"])
        worst = 0.0
        for t, r in R.mp_rows("default"):
            _, (pos, ang) = R.mp_iterate(I.targets()[t], I.seeds()[t][r], k)
            res = R.restatement("default", k)[t][1][r]
            worst = max(worst, abs(res[0] - pos), abs(res[1] - ang))
        assert worst < PIN_BOUND, (k, worst)
    sp = R.special_floors()
    print("special seeds, k = 1, 2, 3: floor_mp", sp["floor_mp"], "floor_f64", sp["floor_f64"])
    assert f["floor_mp"][1] >= sp["floor_mp"][1]
    for k in R.SPECIAL_KS:
        assert sp["floor_mp"][k] < PIN_BOUND and sp["floor_f64"][k] < PIN_BOUND and 0 < sp["gate_mp"][k] == R.MARGIN * max(sp["floor_mp"][k], sp["floor_f64"][k])


def test_b_c_the_noise_floor_of_f64_and_the_gates():
    """2b, 2c. two f64 formulations on all 2048 seeds at k = 1 .. 16; gate = 100 x that floor, gate_mp = 100 x max(floor_mp, floor_f64);
    nothing is hard-coded, and every gate is far below what a mistake moves (PIN_BOUND / 3e-5)"""
    f = R.floors("default")
    print("floor_f64:", f["floor_f64"], "\ngate:", f["gate"], "\ngate_mp:", f["gate_mp"])
    assert f["ks"] == (1, 2, 4, 8, 16) and sum(len(s) for s in R.setting_inputs("default")[1]) == 2048
    for k in f["ks"]:
        assert 0 < f["floor_f64"][k] and f["gate"][k] == 100 * f["floor_f64"][k] < PIN_BOUND, (k, f["floor_f64"])
    for k in f["mp_ks"]:
        assert f["gate_mp"][k] == 100 * max(f["floor_mp"][k], f["floor_f64"][k]) < PIN_BOUND


# rows of the 2048 that a mutant moves by more than 1e-6 rad after ONE step - conditions on the inputs: measured 2048, 2048, 2046, 142,
# 2048, 2048 in this order; the floors are the counts the gates were designed against
MUTANT_ROWS = {"lever": 2048, "lambda": 2048, "l2_scale": 2046, "no_clamp_j6": 67, "error_sign": 2048, "body_frame_error": 2048}


@pytest.mark.parametrize("variant", I.VARIANTS)
def test_d_every_mutant_is_far_above_the_gate(variant):
    """2d. each deliberate mistake, one step, all 2048 seeds: every row it moves at all (> 1e-6 rad) it moves by more than 100 gates, and
    it moves at least the stated number of rows - so a kernel with that mistake fails test_gpu_ik_steps on that many rows"""
    gate = R.floors("default")["gate"][1]
    moved, least = 0, np.inf
    for t in range(I.N_TARGETS):
        d = np.max(np.abs(I.dls_numpy(I.targets()[t], I.seeds()[t], iters=1, variant=variant)[0] - R.restatement("default", 1)[t][0]), axis=1)
        m = d > MOVED
        moved += int(m.sum())
        least = min(least, float(d[m].min()) if m.any() else np.inf)
        assert (d[m] > 100 * gate).all()
    print(f"{variant}: moves {moved} of 2048 rows, the least by {least:.3e} rad; gate[1] = {gate:.3e}")
    assert MOVED > 100 * gate and moved >= MUTANT_ROWS[variant] and least >= 3e-5, (moved, least, gate)
    assert set(MUTANT_ROWS) == set(I.VARIANTS)


def test_the_default_variant_is_the_unchanged_iteration():
    a = I.dls_numpy(I.targets()[1], I.seeds()[1][:16], iters=3)
    b = I.dls_numpy(I.targets()[1], I.seeds()[1][:16], iters=3, variant=None)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        I.dls_numpy(I.targets()[1], I.seeds()[1][:1], iters=1, variant="levr")


def test_e_few_rows_sit_at_the_tolerance():
    """2e. rows whose residual lies within gate[k] of a tolerance may come out on either side of the validity rule on a correct kernel:
    at most 2 of 2048 at k = 8 and at k = 16 (a condition on the inputs; it caps what the GPU comparison of `valid` leaves out)"""
    for k in (8, 16):
        near = R.near_tolerance("default", k)
        valid = np.concatenate([v for _, _, v in R.restatement("default", k)])
        print(f"k = {k}: {int(near.sum())} rows within gate[{k}] = {R.floors('default')['gate'][k]:.3e} of a tolerance; {int(valid.sum())} valid rows")
        assert near.shape == (2048,) and near.sum() <= 2
    assert np.concatenate([v for _, _, v in R.restatement("default", 16)]).sum() >= 8  # the rule is exercised on both sides


@pytest.mark.parametrize("name", [n for n in R.SETTINGS if n != "default"])
def test_the_other_settings_have_floors_and_gates_of_their_own(name):
    """3 targets x 64 seeds, k = 1 and 4, mpmath on 4 seeds each - derived for the setting as 2a-2c - and the condition each setting is
    there for"""
    f = R.floors(name)
    par = R.SETTINGS[name]
    tg, sd = R.setting_inputs(name)
    print(name, "floor_f64", f["floor_f64"], "floor_mp", f["floor_mp"], "gate", f["gate"], "gate_mp", f["gate_mp"])
    assert f["ks"] == (1, 4) and len(sd) == 3 and all(s.shape == (64, 7) for s in sd) and len(R.mp_rows(name)) == 12
    for k in f["ks"]:
        assert 0 < f["floor_f64"][k] < PIN_BOUND and 0 < f["floor_mp"][k] < PIN_BOUND
        assert f["gate"][k] == 100 * f["floor_f64"][k] and f["gate_mp"][k] == 100 * max(f["floor_mp"][k], f["floor_f64"][k]) < MOVED
    big = np.concatenate([R.dls_cholesky(tg[t], sd[t], iters=4, return_big=True, **par)[1] for t in range(3)], axis=1)  # (4, 192)
    scaled = big > par["max_step"]
    print(name, "rows scaled per iteration:", scaled.sum(axis=1).tolist(), "of 192")
    if name == "damped_small_steps":
        assert scaled.all()
    if name == "light_large_steps":
        # meant as "almost none scaled"; measured: from seeds drawn over the whole joint range the lightly damped step exceeds even 2 rad
        # on 158, 140, 124, 105 of the 192 rows in iterations 1-4.  What the setting does give, and what is asserted: the only setting in
        # which a good share of the rows takes the UNSCALED branch far from the solution, in every iteration
        assert ((~scaled).sum(axis=1) >= 32).all() and scaled.any(axis=1).all()
    if name in ("flange", "custom"):  # posed in the setting's own frame: the frames differ by far more than any gate
        assert np.linalg.norm(tg[0][:3, 3] - I.targets()[0][:3, 3]) > 0.05
        assert max(I.pose_error(I.fk(I.target_configurations()[0], par["tool"]), tg[0])) < 1e-15
