"""The corner-blend rule (tests/blend_inputs.py) against things that are independent of it, on the CPU: a linear programme for the waypoint
speeds, a dense evaluation of the blended motion for the limit, continuity and deviation properties - and what each step of the rule is
for, shown by leaving it out.  Plus the presence of the four entry points (include/edmp_hip.h, _capi.SIGNATURES, the library) and the
durations before and after blending on four input families (informative: printed, and written as JSON where EDMP_BLEND_DURATIONS_OUT
names a file - profiles/blend_durations.json comes from such a run)."""
import json
import math
import os
import re

import numpy as np
import pytest

from edmp_amd import _capi
from tests import blend_inputs as I
from tests import timing_inputs as TI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = I.far_obstacles(1, 0)


def timed_rows(names=None):
    """(case name, row index, x, blended profile, case) of every timed (finite) row"""
    for name in I.names():
        if names is not None and name not in names:
            continue
        c = I.case(name)
        for r, prof in enumerate(c["prof"]["rows"]):
            if math.isfinite(prof["duration"]):
                yield name, r, c["X"][r], prof, c


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "edmp_hip.h")).read(), flags=re.S)
    lib = _capi.load()
    for name, nargs in (("edmp_blend_rows_dev", 18), ("edmp_scenes_blend_rows_dev", 19), ("edmp_time_blended_rows_dev", 15), ("edmp_sample_blended_rows_dev", 17)):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in _capi.SIGNATURES and hasattr(lib, name) and len(_capi.SIGNATURES[name][1]) == nargs, name
    assert '"blend.hip"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_every_case_is_admitted_and_the_cases_cover_what_they_are_for():
    """case() asserts the admission of each; here: the probes do what their docstrings say; the named cases give the codes they are named
    for; every code -1..4, N = 2, 3, 4, 5, 50, 64, 1..9 rows, K_b = 1, 4, 8, H = 0..3, 1 / 7 / 64 obstacles with cylinders, halved = 0, 1, 2
    and both limit meanings of code 3 occur"""
    pat = I.check_probes()
    assert pat["cube"].tolist() == pat["cylinder"].tolist() == [False] * 4 + [True] + [False] * 4 and pat["end"].tolist() == [False] * 8 + [True]
    codes, halved, Ns, ns, Ks, Hs, nos = set(), set(), set(), set(), set(), set(), set()
    for name in I.names():
        c = I.case(name)
        ok, why, _, _ = I.admit(c["X"], c["obstacle_config"], c["kinds"], c["limits"], c["deviation"], c["reach"], c["Kb"], c["H"])
        assert ok, (name, why)
        ref = c["ref"]
        codes.update(ref["code"].reshape(-1).tolist())
        halved.update(ref["halved"][ref["code"] == 3].tolist())
        ns.add(c["X"].shape[0]), Ns.add(c["X"].shape[2]), Ks.add(c["Kb"]), Hs.add(c["H"])
        nos.add((len(c["kinds"]), bool((c["kinds"] == 1).any())))
        if name in I.EXPECT:
            e = I.EXPECT[name]
            assert ref["code"].tolist() == e["code"] and ref["halved"].tolist() == e["halved"] and ref["tested"].tolist() == e["tested"], name
        assert (ref["halved"][ref["code"] != 3] == 0).all() and (ref["beta"][ref["code"] != 3] == 0).all() if -1 not in ref["code"] else True
    assert codes == {-1, 0, 1, 2, 3, 4} and halved >= {0, 1, 2} and Ns >= {2, 3, 4, 5, 50, 64} and ns >= set(range(1, 10))
    assert Ks >= {1, 4, 8} and Hs >= {0, 1, 2, 3} and {(1, False), (7, True), (64, True)} <= nos
    # the middle configuration alone decides: at K_b = 1 it is not tested and the blend is taken at beta0; the end alone decides: below
    mid, k1 = I.case("L_middle_decides_h1_passes"), I.case("L_middle_untested_at_K1")
    (i, h, b, hk), = [t for t in mid["ref"]["runs"][0]["tries"] if t[1] == 0]
    assert hk.tolist() == [False, False, True, False, False] and k1["ref"]["beta"][0, 1] == b == I.L_BETA0
    (i, h, b, hk), = [t for t in I.case("L_end_decides_o64")["ref"]["runs"][0]["tries"] if t[1] == 0]
    assert hk.tolist() == [False, False, False, False, True]
    pair = I.case("pair_N4_n8_both_at_reach_045")
    assert (pair["ref"]["beta"][:, 1:3] == 0.45).all() and np.allclose(pair["prof"]["rows"][0]["ell"], [0.55, 0.1, 0.55], atol=1e-15)
    zeros = I.case("zeros_N8_n3_start_middle_pair")["ref"]["code"]
    assert zeros[0, 1] == 0 and zeros[1, 3] == 0 and zeros[1, 4] == 0 and zeros[2, 2:5].tolist() == [0, 0, 0]  # beside a repeated waypoint: none
    chord = I.case("chord_N50_n1_collinear_run")["ref"]["code"][0]
    assert set(chord[7:45].tolist()) <= {0, 1} and chord[6] == 3 and chord[45] == 3  # inside the run: no corner, or a rounding of one
    still = I.case("still_N5_n1")
    assert not still["ref"]["code"].any() and still["prof"]["duration"].tolist() == [0.0]
    nan = I.case("nan_N50_n3")
    assert (nan["ref"]["code"][1] == -1).all() and np.isnan(nan["ref"]["beta"][1]).all() and np.isnan(nan["prof"]["duration"][1])
    lim3 = [(float(p["beta"][i]) > 0) for _, _, _, p, _ in timed_rows() for i in np.nonzero(p["limit"] == 3)[0]]
    assert any(lim3) and not all(lim3)


@pytest.mark.parametrize("name", ["walk_N50_n9_o7c2", "pair_N4_n8_both_at_reach_045", "zeros_N8_n3_start_middle_pair", "coarse_N5_n6_o7c2_H3", "chord_N50_n1_collinear_run",
                                  "L_middle_decides_h1_passes"])
def test_waypoint_speeds_are_the_maximum_of_a_linear_programme(name):
    """y = argmax sum y_i subject to 0 <= y_i <= c_i, |y_{i+1} - y_i| <= 2 A_i l_i (a zero segment: y_{i+1} = y_i), solved by HiGHS in units
    of the row's largest finite bound - the solver tests/test_timing_host.py uses.  Gate: the solver's feasibility tolerance 1e-7 per
    constraint of the longest chain, N of them."""
    from scipy.optimize import linprog

    for _, r, x, prof, _ in timed_rows({name}):
        N = x.shape[1]
        c = np.min(prof["cands"][:, :4], axis=1)
        step = 2.0 * prof["A"] * prof["ell"]
        bound = np.concatenate([c[np.isfinite(c)], step[np.isfinite(step)]])
        unit = float(bound.max())
        rows, rhs, eq, eq_rhs = [], [], [], []
        for i in range(N - 1):
            e = np.zeros(N)
            e[i + 1], e[i] = 1.0, -1.0
            if prof["zero"][i]:
                eq.append(e)
                eq_rhs.append(0.0)
            else:
                rows += [e, -e]
                rhs += [step[i] / unit] * 2
        res = linprog(-np.ones(N), A_ub=np.array(rows) if rows else None, b_ub=np.array(rhs) if rows else None, A_eq=np.array(eq) if eq else None,
                      b_eq=np.array(eq_rhs) if eq else None, bounds=[(0.0, ci / unit if math.isfinite(ci) else None) for ci in c], method="highs")
        assert res.status == 0, res.message
        err = float(np.abs(res.x * unit - prof["y"]).max()) / unit
        print(f"[blend lp] {name} row {r}: N = {N}, max |y_rule - y_lp| = {err:.3e} of the largest bound, gate {N * 1e-7:.1e}")
        assert err <= N * 1e-7, (name, r, err)


def test_properties_hold_on_a_dense_evaluation():
    """on every timed row of every case: |qdot_j| <= vmax_j, |qddot_j| <= amax_j (straight parts and blends), position continuous at every
    piece boundary, velocity continuous at a blended corner and its jump <= jump_j at an unblended one, every blend point within deviation_j
    of the matched point of the polyline, and the motion ends at the goal at rest.  Allowances: 1e-9 on the ratios (formed from the rule's
    rounded numbers); 1e-12 rad on positions; 1e-9 of jump_j on the velocity at a blended corner (the issue's experiment saw 3e-12); rows with
    a zero segment are left out of the unblended-jump figure (two capped jumps meet at a repeated waypoint)."""
    worst = dict(speed=0.0, accel=0.0, position_gap=0.0, velocity_gap_blended=0.0, velocity_gap_unblended=0.0, deviation=0.0, end=0.0)
    n = 0
    for name, r, x, prof, c in timed_rows():
        v = I.dense_check(x, prof, c["limits"], c["deviation"])
        if prof["zero"].any():
            v["velocity_gap_unblended"] = 0.0
        worst = {k: max(worst[k], v[k]) for k in worst}
        assert v["speed"] <= 1 + 1e-9 and v["accel"] <= 1 + 1e-9 and v["velocity_gap_unblended"] <= 1 + 1e-9 and v["deviation"] <= 1 + 1e-9, (name, r, v)
        assert v["position_gap"] <= 1e-12 and v["velocity_gap_blended"] <= 1e-9 and v["end"] <= 1e-9, (name, r, v)
        n += 1
    print(f"[blend properties] {n} rows", worst)
    assert n >= 60 and worst["speed"] > 0.999 and worst["accel"] > 0.999 and worst["deviation"] > 0.99 and worst["velocity_gap_unblended"] > 0.999


def test_binding_only_rule_left_out_slows_gently_curved_rows():
    """blending the corners whose cap does not bind as well makes every gently curved row (the straight line between two far-apart
    configurations plus a half-sine bump of at most 0.02 rad per joint, 50 waypoints: J^2 >= V^2 at every corner, yet (2 beta) K > J^2 at
    most) slower, one of the four by more than 5 %: a blend is crossed at constant speed, so forty of them at beta = 0.4 leave the row a
    fifth of its length to accelerate on.  On the collinear runs themselves - Delta a rounding - the step changes nothing, because there
    the gain rule refuses the blend as well (J^2 is many orders above (2 beta) K): that is asserted too."""
    from tests import shortcut_inputs as SI

    ends, ratios = TI.coarse_rows(23, 4, 2), []
    for r in range(4):
        x = SI.bumped_rows(dict(start=ends[r, :, 0], goal=ends[r, :, 1]), 1, 50, 0.02, 3 + r)[0]
        rule = I.blend_row(x, *FAR, I.LIMITS, 0.02, 0.4, 4, 2)
        every = I.blend_row(x, *FAR, I.LIMITS, 0.02, 0.4, 4, 2, binding_only=False)
        a, b = (I.time_blended_row(x, run["beta"], *I.LIMITS)["duration"] for run in (rule, every))
        print(f"[blend binding-only] bumped row {r}: {int((rule['code'] == 3).sum())} blends {a:.4f} s; with every corner {int((every['code'] == 3).sum())} blends {b:.4f} s")
        assert set(rule["code"][1:-1].tolist()) == {1} and a == TI.time_row(x, *I.LIMITS)["duration"] and (every["code"] == 3).sum() >= 40 and b > a * (1 + 1e-5), (r, a, b)
        ratios.append(b / a)
    assert max(ratios) > 1.05, ratios
    for r, x in enumerate(I.collinear_rows(42, 4)):
        rule = I.blend_row(x, *FAR, I.LIMITS, 0.02, 0.4, 4, 2)
        every = I.blend_row(x, *FAR, I.LIMITS, 0.02, 0.4, 4, 2, binding_only=False)
        assert np.array_equal(rule["beta"], every["beta"]) and set(every["code"][rule["code"] == 1].tolist()) == {2}, r


def test_gain_rule_left_out_lowers_a_corner_cap_below_the_jump_cap():
    """L_hit_then_no_gain_at_h1 without the gain rule: the halved blend passes the test and is taken, its cap (2 beta) K lies below J^2, and
    the row is slower than with the corner left alone"""
    c = I.case("L_hit_then_no_gain_at_h1")
    x = c["X"][0]
    run = I.blend_row(x, c["obstacle_config"], c["kinds"], c["limits"], c["deviation"], c["reach"], c["Kb"], c["H"], gain_rule=False)
    t = I.corner_terms(x, 1, *c["limits"])
    assert run["code"][1] == 3 and run["halved"][1] == 1 and (2.0 * run["beta"][1]) * t["K"] < t["J2"]
    assert I.time_blended_row(x, run["beta"], *c["limits"])["duration"] > c["prof"]["duration"][0]


def test_halving_left_out_blocks_a_corner_that_a_smaller_blend_clears():
    c, c0 = I.case("L_middle_decides_h1_passes"), I.case("L_middle_decides_H0_blocked")
    assert c0["ref"]["code"][0, 1] == 4 and c["ref"]["code"][0, 1] == 3 and c["prof"]["duration"][0] < c0["prof"]["duration"][0]


def test_untested_configurations_miss_a_hit():
    """the end configurations k = 0 and k = K_b left out: the blend of L_end_decides_o64 is taken at beta0, and its end configuration - a
    point of the polyline between two of the success check's substeps - hits.  Likewise the middle at K_b = 1 (a case of its own: the
    guarantee covers the K_b + 1 configurations, nothing between them)."""
    c = I.case("L_end_decides_o64")
    x = c["X"][0]
    run = I.blend_row(x, c["obstacle_config"], c["kinds"], c["limits"], c["deviation"], c["reach"], c["Kb"], c["H"], ends=False)
    assert run["code"][1] == 3 and run["halved"][1] == 0 and run["tested"] == 3
    assert I.hits(I.blend_config(x, 1, run["beta"][1], 1.0)[None], c["obstacle_config"], c["kinds"])[0]
    assert c["ref"]["halved"][0, 1] == 1 and not I.hits(np.array([I.blend_config(x, 1, c["ref"]["beta"][0, 1], k / 4) for k in range(5)]), c["obstacle_config"], c["kinds"]).any()
    k1 = I.case("L_middle_untested_at_K1")
    assert I.hits(I.blend_config(k1["X"][0], 1, k1["ref"]["beta"][0, 1], 0.5)[None], k1["obstacle_config"], k1["kinds"])[0]


def test_beta_zero_gives_the_unblended_rule_exactly():
    """time_blended_row with beta = 0 has timing_inputs.time_row's bits in every common output, times[i] = (T_i, T_i), and the motion's samples
    are timing_inputs.sample_row's bits"""
    def bits(a):
        return np.ascontiguousarray(a).view(np.int64 if np.asarray(a).dtype == np.float64 else np.int32)

    for name in TI.names():
        c = TI.case(name)
        for r, x in enumerate(c["X"]):
            old = c["ref"]["rows"][r]
            new = I.time_blended_row(x, np.zeros(x.shape[1]), *c["limits"])
            for k in ("y", "phase", "limit", "seg", "cands"):
                assert np.array_equal(bits(new[k]), bits(old[k])), (name, r, k)
            assert np.array_equal(bits(new["times"][:, 0]), bits(old["times"])) and np.array_equal(bits(new["times"][:, 1]), bits(old["times"]))
            assert np.array_equal(bits(np.float64(new["duration"])), bits(np.float64(old["duration"]))) and (not math.isfinite(old["duration"]) or not new["blend"].any())
            if math.isfinite(old["duration"]) and x.shape[1] <= 8:
                period = old["duration"] / 40.5 if old["duration"] > 0 else 1e-3
                a, b = I.sample_row(x, new, period, 44), TI.sample_row(x, old, period, 44)
                assert np.array_equal(bits(a["q"]), bits(b["q"])) and np.array_equal(bits(a["qd"]), bits(b["qd"])) and a["count"] == b["count"], (name, r)


def test_motion_starts_at_the_start_holds_the_goal_and_never_goes_back():
    c = I.case("pair_N4_n8_both_at_reach_045")
    x, prof = c["X"][0], c["prof"]["rows"][0]
    period = I.choose_period([prof], 200.5)
    smp = I.sample_row(x, prof, period, 204)
    assert smp["count"] == 202 and np.array_equal(smp["q"][:, 0], x[:, 0]) and not smp["qd"][:, 0].any()
    assert np.array_equal(smp["q"][:, 201:].view(np.int64), np.repeat(x[:, 3:4], 3, axis=1).view(np.int64)) and not smp["qd"][:, 201:].any()
    assert (np.diff(smp["piece"]) >= 0).all() and set(smp["piece"][:201].tolist()) == {0, 1, 2, 3, 4}
    for p in range(5):
        par = smp["parameter"][:201][smp["piece"][:201] == p]
        assert (np.diff(par) >= 0).all() and par.min() >= 0 and par.max() <= 1


def test_durations_before_and_after_blending():
    """informative: the median duration of each family unblended and blended at 1 / 5 / 20 / 50 mrad, reach 0.4, K_b = 4, H = 2, no obstacle
    near (nothing is blocked) - printed, and written where EDMP_BLEND_DURATIONS_OUT says.  Asserted: only that blending under the rule
    never makes a row of these families slower by more than a rounding."""
    table = {}
    for fam, X in I.families().items():
        base = np.array([TI.time_row(x, *I.LIMITS)["duration"] for x in X])
        row = {"rows": int(X.shape[0]), "N": int(X.shape[2]), "unblended_median_s": float(np.median(base)), "blended_median_s": {}, "blends_per_row": {}}
        for dev in (0.001, 0.005, 0.02, 0.05):
            runs = [I.blend_row(x, *FAR, I.LIMITS, dev, 0.4, 4, 2) for x in X]
            dur = np.array([I.time_blended_row(x, run["beta"], *I.LIMITS)["duration"] for x, run in zip(X, runs)])
            row["blended_median_s"][f"{dev * 1e3:g} mrad"] = float(np.median(dur))
            row["blends_per_row"][f"{dev * 1e3:g} mrad"] = float(np.mean([(run["code"] == 3).sum() for run in runs]))
            assert (dur <= base * (1 + 1e-12)).all(), (fam, dev, dur, base)
        table[fam] = row
        print(f"[blend durations] {fam}: unblended {row['unblended_median_s']:.3f} s; blended " + ", ".join(f"{v:.3f} s at {k}" for k, v in row["blended_median_s"].items()))
    out = os.environ.get("EDMP_BLEND_DURATIONS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"what": "median duration of the host rule's motion before and after blending (tests/test_blend_host.py), default limits, reach 0.4, "
                               "substeps 4, halvings 2, no obstacle near; informative, not a gate", "families": table}, f, indent=1)
            f.write("\n")
