"""The time parameterisation's rule (tests/timing_inputs.py) against things that are independent of it, on the CPU: a linear programme for
the waypoint speeds, a numerical quadrature for the phase times, a dense evaluation for the limit properties - and what each step of the
rule is for, shown by leaving it out.  Plus the presence of the two entry points (include/edmp_hip.h, _capi.SIGNATURES, the library)."""
import math
import os
import re

import numpy as np
import pytest

from edmp_amd import _capi, franka
from edmp_amd import evaluation as E
from tests import timing_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMED = [(name, r) for name in I.names() for r in range(I.case(name)["X"].shape[0])]


def timed_rows(names=None):
    """(case name, row index, x, profile, limits) of every timed (finite) row"""
    for name, r in TIMED:
        c = I.case(name)
        prof = c["ref"]["rows"][r]
        if (names is None or name in names) and math.isfinite(prof["duration"]):
            yield name, r, c["X"][r], prof, c["limits"]


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "edmp_hip.h")).read(), flags=re.S)
    lib = _capi.load()
    for name in ("edmp_time_rows_dev", "edmp_sample_rows_dev"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert "#define EDMP_MAX_TIMED_SAMPLES %d " % _capi.MAX_TIMED_SAMPLES in open(os.path.join(ROOT, "include", "edmp_hip.h")).read()
    assert "timing.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_default_limits():
    vm, am, jm = franka.timing_limits()
    assert vm.tolist() == [2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61] and am.tolist() == [15, 7.5, 10, 12.5, 15, 20, 20]
    assert jm.tolist() == [a * 1e-3 for a in am.tolist()]
    vs, as_, js = franka.timing_limits(scale=(0.5, 0.25))
    assert np.array_equal(vs, vm * 0.5) and np.array_equal(as_, am * 0.25) and np.array_equal(js, jm)
    for bad in (dict(vmax=[1.0] * 6), dict(amax=[0.0] * 7), dict(jump=[float("nan")] * 7), dict(scale=(-1, 1))):
        with pytest.raises(ValueError):
            franka.timing_limits(**bad)


def test_every_case_is_admitted_and_the_cases_cover_what_they_are_for():
    """no `limit` code of a case sits on a rounding; each code 1-5 binds somewhere; N = 2, 3, 4, 50, 64; n = 1, 2, 3, 4, 5, 9; a cruising and
    a triangular segment; zero segments at the start, in the middle and two in a row; start = goal throughout; a NaN row"""
    codes, Ns, ns = set(), set(), set()
    for name in I.names():
        c = I.case(name)
        ns.add(c["X"].shape[0])
        Ns.add(c["X"].shape[2])
        for r, prof in enumerate(c["ref"]["rows"]):
            ok, gap = I.admit(prof)
            assert ok, (name, r, gap)
            codes.update(prof["limit"].tolist())
    assert codes == {-1, 0, 1, 2, 3, 4, 5} and Ns >= {2, 3, 4, 50, 64} and ns >= {1, 2, 3, 4, 5, 9}
    two = I.case("two_N2_n2_cruise_and_triangle")["ref"]["phase"]
    assert two[0, 0, 1] > 0 and two[1, 0, 1] == 0 and two[1, 0, 0] > 0 and two[1, 0, 2] > 0
    z = [p["zero"].tolist() for p in I.case("zeros_N8_n3_start_middle_pair")["ref"]["rows"]]
    assert z[0] == [True] + [False] * 6 and z[1] == [False] * 3 + [True] + [False] * 3 and z[2] == [False, False, True, True, False, False, False]
    for name in ("still_N5_n1", "still_N2_n1"):
        ref = I.case(name)["ref"]
        assert ref["duration"].tolist() == [0.0] and not ref["y"].any() and not ref["phase"].any() and I.sample_count(0.0, 1e-3) == 1
    nan = I.case("nan_N50_n3")["ref"]
    assert np.isnan(nan["duration"]).tolist() == [False, True, False] and (nan["limit"][1] == -1).all() and np.isnan(nan["y"][1]).all()
    chord = I.case("chord_N50_n1")
    assert set(chord["ref"]["limit"][0, 7:45].tolist()) <= {4, 5}  # collinear: no corner cap inside the chord


@pytest.mark.parametrize("name", ["coarse_N3_n3", "zeros_N8_n3_start_middle_pair", "walk_N50_n9", "walk_N64_n5_big_jump", "chord_N50_n1", "coarse_N4_n4_big_jump"])
def test_waypoint_speeds_are_the_maximum_of_a_linear_programme(name):
    """y = argmax sum y_i subject to 0 <= y_i <= c_i, |y_{i+1} - y_i| <= 2 A_i (a zero segment: y_{i+1} = y_i), solved by HiGHS in units of
    the row's largest finite bound.  Gate: the solver's feasibility tolerance 1e-7 (absolute, in those units) per constraint of the longest
    chain, N of them - nothing of the rule's own error enters."""
    from scipy.optimize import linprog

    for _, r, x, prof, _ in timed_rows({name}):
        N = x.shape[1]
        c = np.min(prof["cands"][:, :4], axis=1)
        bound = np.concatenate([c[np.isfinite(c)], 2.0 * prof["A"][np.isfinite(prof["A"])]])
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
                rhs += [2.0 * prof["A"][i] / unit] * 2
        res = linprog(-np.ones(N), A_ub=np.array(rows) if rows else None, b_ub=np.array(rhs) if rows else None, A_eq=np.array(eq) if eq else None,
                      b_eq=np.array(eq_rhs) if eq else None, bounds=[(0.0, ci / unit if math.isfinite(ci) else None) for ci in c], method="highs")
        assert res.status == 0, res.message
        err = float(np.abs(res.x * unit - prof["y"]).max()) / unit
        print(f"[timing lp] {name} row {r}: N = {N}, max |y_rule - y_lp| = {err:.3e} of the largest bound, gate {N * 1e-7:.1e}")
        assert err <= N * 1e-7, (name, r, err)


def test_phase_times_equal_a_quadrature_of_ds_over_sdot():
    """each phase's time = integral ds / sqrt y(s) over its part of the bang-cruise-bang profile y(s) = y_i + 2 A s | p | y_{i+1} + 2 A (1 - s),
    by QUADPACK's adaptive rule (scipy.integrate.quad, asked for 1e-13 relative) in u = sqrt(distance from the phase's slow end), which takes
    the 1 / sqrt singularity of a rest end out: the integrand 2 u / sqrt(y0 + 2 A u^2) is bounded by sqrt(2 / A).  Gate: 4 x the quadrature's
    own error estimate plus 1e-12 of the segment's time plus 1e-15 s (the rule's three times carry a handful of roundings each)."""
    from scipy.integrate import quad as quadpack

    worst, n = 0.0, 0
    for name, r, x, prof, _ in timed_rows():
        for i in range(x.shape[1] - 1):
            if prof["zero"][i]:
                assert not prof["phase"][i].any()
                continue
            A, p = (float(v) for v in prof["seg"][i])
            total = float(prof["phase"][i].sum())
            for k, y0 in ((0, float(prof["y"][i])), (2, float(prof["y"][i + 1]))):
                length = max(0.0, (p - y0) / (2.0 * A))  # the phase's extent in s
                quad, est = quadpack(lambda u: 2.0 * u / math.sqrt(y0 + 2.0 * A * u * u), 0.0, math.sqrt(length), epsabs=0.0, epsrel=1e-13, limit=200) if length > 0 else (0.0, 0.0)
                worst, n = max(worst, abs(quad - prof["phase"][i, k]) / (4.0 * est + 1e-12 * total + 1e-15)), n + 1
            cruise = max(0.0, 1.0 - (p - float(prof["y"][i])) / (2.0 * A) - (p - float(prof["y"][i + 1])) / (2.0 * A)) / math.sqrt(p)
            worst = max(worst, abs(cruise - prof["phase"][i, 1]) / (1e-12 * total + 1e-15))
            # a cruise phase runs at V_i (a triangular segment may carry a cruise "phase" of a rounding's length)
            assert p <= prof["V2"][i] and (prof["phase"][i, 1] <= 1e-12 * total or p == prof["V2"][i])
    print(f"[timing quadrature] {n} phases, worst error / gate = {worst:.3e}")
    assert n > 500 and worst <= 1.0, worst


def test_limit_properties_hold_on_a_dense_evaluation():
    """|qdot_j| <= vmax_j, |qddot_j| <= amax_j inside segments, the velocity jump at a waypoint <= jump_j, and every segment's motion ends on
    s = 1 at sqrt y_{i+1}.  Allowance 1e-9: the ratios are formed from the rule's rounded numbers."""
    worst = dict(speed=0.0, accel=0.0, jump=0.0, closure=0.0)
    for name, r, x, prof, lim in timed_rows():
        v = I.violations(x, prof, *lim)
        worst = {k: max(worst[k], v[k]) for k in worst}
        assert v["speed"] <= 1 + 1e-9 and v["accel"] <= 1 + 1e-9 and v["jump"] <= 1 + 1e-9 and v["closure"] <= 1e-9, (name, r, v)
    print("[timing properties]", worst)
    assert worst["speed"] > 0.999 and worst["accel"] > 0.999 and worst["jump"] > 0.999  # every limit is reached somewhere: the optimum


@pytest.mark.parametrize("step,names,broken", [("corner", ("walk_N50_n9", "coarse_N3_n3"), "jump"), ("backward", ("walk_N64_n5_big_jump", "chord_N50_n1"), "closure"),
                                               ("cruise", ("two_N2_n2_cruise_and_triangle", "coarse_N4_n4_big_jump"), "speed")])
def test_each_step_left_out_breaks_a_property(step, names, broken):
    """the rule without the corner cap, without the backward pass, without the cruise clamp violates the property that step is there for, on
    every row of that step's cases that exercises it"""
    hit = 0
    for name, r, x, prof, lim in timed_rows(set(names)):
        if step == "cruise" and not prof["phase"][:, 1].any():
            continue  # (the triangular row has nothing to clamp)
        v = I.violations(x, I.time_row(x, *lim, **{step: False}), *lim)
        assert (v[broken] > 1.01) if broken != "closure" else (v[broken] > 1e-3), (name, r, step, v)
        hit += 1
    assert hit >= 2


def test_count_rule_at_exact_multiples_of_the_period():
    """count = 1 + the smallest k with float(k) * period >= duration, where float(k) * period is the product as the sampler forms it - not
    k = ceil(duration / period), which is off by one where the quotient rounds across an integer.  The package's statement
    (evaluation.sample_count) and the test rule's agree."""
    for period in (1e-3, 0.1, 1.0 / 3.0, 0.004, 7e-4):
        for k in (0, 1, 2, 3, 7, 10, 255, 256, 257, 1000, 1025, 12345):
            d = float(k) * period
            for dur in (d, np.nextafter(d, np.inf), np.nextafter(d, -np.inf) if k else 0.0):
                want = 1 + next(m for m in range(max(k - 2, 0), k + 3) if float(m) * period >= dur)
                assert I.sample_count(dur, period) == want == E.sample_count(dur, period), (period, k, dur)
            assert I.sample_count(d, period) == k + 1
    assert I.sample_count(float("nan"), 1e-3) == 0 == E.sample_count(float("nan"), 1e-3)


def test_motion_holds_the_goal_and_stays_on_the_polyline():
    """host closed form: q(0) = start, t >= duration gives the goal's bits at rest, s is non-decreasing inside every segment"""
    c = I.case("coarse_N4_n4_big_jump")
    x, prof = c["X"][0], c["ref"]["rows"][0]
    smp = I.sample_row(x, prof, prof["duration"] / 200.5, 204)
    assert smp["count"] == 202 and np.array_equal(smp["q"][:, 0], x[:, 0]) and not smp["qd"][:, 0].any()
    assert np.array_equal(smp["q"][:, 201:].view(np.int64), np.repeat(x[:, 3:4], 3, axis=1).view(np.int64)) and not smp["qd"][:, 201:].any()
    path = smp["segment"] + smp["s"]
    assert (np.diff(path) >= -1e-12).all() and (smp["s"] >= 0).all() and (smp["s"] <= 1).all()
