"""The time parameterisation (time_rows_kernel, sample_rows_kernel; edmp_time_rows_dev, edmp_sample_rows_dev) on the GPU against the rule of
tests/timing_inputs.py on admitted cases, and against itself where the property is bit-equality.

Gates, all derived from the number format and the shapes (R = roundings in the longest chain of the quantity):
  limit, count         exactly
  y                    4 R 2^-53 of the row's largest y, R = N + 8        (N - 1 transfers of one add each, and the bounds in front of them)
  phase, times         4 R 2^-53 of the row's duration, R = 3 (N - 1) + 16 (three adds per segment, and the phase's own operations)
  q                    vmax_j x (the time gate, in seconds) + 64 x 2^-53 max |x|: a time error moves a sample along the path by at most its
                       speed; the rest is the interpolation's own rounding
  qd                   amax_j x (the time gate) + 64 x 2^-53 vmax_j: the same argument one derivative up
Every comparison prints its error and gate and says whether the equality was in fact bit for bit; with EDMP_TIMING_PARITY_OUT=<file> the
records are written there as JSON (profiles/timing_parity.json comes from such a run)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from edmp_amd import _capi, franka
from edmp_amd import evaluation as E
from tests import repair_inputs as RI
from tests import sdf_reference as R
from tests import timing_inputs as I
from tests.sdf_gpu import DEV, recorder, run_cfgs, tiny_net  # noqa: F401  (tiny_net: this module's fixture)
from tests.sdf_term_suite import segmented_run_goes_on

pytestmark = pytest.mark.gpu
record, _write_records = recorder("timing parity", "EDMP_TIMING_PARITY_OUT",
                                  "limit and count exactly; y within 4 (N + 8) 2^-53 of the row's largest y; phase and times within 4 (3 (N - 1) + 16) 2^-53 of the "
                                  "row's duration; q within vmax_j x that time gate + 64 x 2^-53 max |x|; qd within amax_j x that time gate + 64 x 2^-53 vmax_j")
EPS = 2.0 ** -53
PROFILE = E.PROFILE_KEYS
SAMPLES = ("q", "qd", "count")


def bits(a):
    """raw bits, NaN patterns included"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same(a, b, keys):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def make_guide(seed, n, no=4, device=DEV):
    """a guide over a random scene with n plain rows: the timing calls read nothing of it but its context"""
    from edmp_amd.guide import IntersectionVolumeGuide

    inp, cfgs = R.make_case(seed, n, 12, no, 0), RI.plain_cfgs(n)
    return IntersectionVolumeGuide(inp["obstacle_config"], device, cfgs, cfgs["total_batch_size"], link_mesh_extents=franka.PLACEHOLDER_LINK_EXTENTS,
                                   obstacle_kinds=inp["kinds"]), inp


def period_of(ref, samples=300.5):
    """a period that gives about `samples` samples for the case's longest row (1 ms for a case that does not move)"""
    d = np.nanmax(ref["duration"])
    return float(d) / samples if d > 0 else 1e-3


@pytest.mark.parametrize("name", I.names())
def test_against_the_rule(name):
    """every case through both kernels: limit and count exactly, y / phase / times / samples inside their derived gates; the last sample
    and every held sample are the goal's bits at rest; every sample lies on its segment and the recovered path parameter never decreases;
    central differences of q agree with qd within amax_j period + jump_j"""
    c = I.case(name)
    X, ref, (vmax, amax, jump) = c["X"], c["ref"], c["limits"]
    n, _, N = X.shape
    prof = E.time_rows(X, vmax, amax, jump, device=DEV)
    assert prof["limit"].dtype == np.int32 and np.array_equal(prof["limit"], ref["limit"])
    timed = np.isfinite(ref["duration"])
    for k in ("y", "phase", "times", "seg"):
        assert np.isnan(prof[k][~timed]).all() and np.isfinite(prof[k][timed]).all(), k
    assert np.array_equal(np.isnan(prof["duration"]), ~timed)
    ymax = np.array([np.max(ref["y"][r]) if timed[r] else 0.0 for r in range(n)])
    dur = np.where(timed, ref["duration"], 0.0)
    gate_y, gate_t = 4 * (N + 8) * EPS * ymax, 4 * (3 * (N - 1) + 16) * EPS * dur
    err_y = np.array([np.abs(prof["y"][r] - ref["y"][r]).max() if timed[r] else 0.0 for r in range(n)])
    err_t = np.array([max(np.abs(prof["phase"][r] - ref["phase"][r]).max(), np.abs(prof["times"][r] - ref["times"][r]).max(),
                          abs(prof["duration"][r] - ref["duration"][r])) if timed[r] else 0.0 for r in range(n)])
    exact = same(prof, ref, PROFILE)
    record(test="rule: profile", case=name, rows=n, N=N, y_abs_err=float(err_y.max()), y_gate=float(gate_y.max()), time_abs_err=float(err_t.max()),
           time_gate=float(gate_t.max()), bit_for_bit=bool(exact), limits_equal=True)
    assert (err_y <= gate_y).all(), (err_y, gate_y)
    assert (err_t <= gate_t).all(), (err_t, gate_t)

    period = period_of(ref)
    out = E.sample_rows(X, prof, period, device=DEV)
    counts = np.array([I.sample_count(d, period) for d in ref["duration"]], dtype=np.int32)
    M = max(1, int(counts.max()))
    assert out["q"].shape == (n, 7, M) and out["qd"].shape == (n, 7, M) and out["count"].dtype == np.int32 and np.array_equal(out["count"], counts)
    assert np.array_equal(out["t"], np.arange(M) * period)
    err_q = err_v = ratio = 0.0
    exact_s = True
    for r in range(n):
        q, qd = out["q"][r], out["qd"][r]
        if not timed[r]:
            assert np.isnan(q).all() and np.isnan(qd).all()
            continue
        smp = I.sample_row(X[r], ref["rows"][r], period, M)
        gq = vmax * gate_t[r] + 64 * EPS * np.abs(X[r]).max()
        gv = amax * gate_t[r] + 64 * EPS * vmax
        eq, ev = np.abs(q - smp["q"]).max(axis=1), np.abs(qd - smp["qd"]).max(axis=1)
        err_q, err_v, ratio = max(err_q, float(eq.max())), max(err_v, float(ev.max())), max(ratio, float((eq / gq).max()), float((ev / gv).max()))
        exact_s = exact_s and np.array_equal(bits(q), bits(smp["q"])) and np.array_equal(bits(qd), bits(smp["qd"]))
        assert (eq <= gq).all() and (ev <= gv).all(), (r, eq, gq, ev, gv)
        held = counts[r] - 1
        assert np.array_equal(bits(q[:, held:]), bits(np.repeat(X[r][:, N - 1:], M - held, axis=1))) and not qd[:, held:].any(), r
        assert np.array_equal(bits(q[:, 0]), bits(X[r][:, 0])) and not qd[:, 0].any(), r
        on_the_polyline(X[r], q, smp["segment"], r)
        cd = (q[:, 2:] - q[:, :-2]) / (2.0 * period)  # central differences against the velocities
        slack = amax * period + jump + 8 * EPS * np.abs(X[r]).max() / period
        assert M < 3 or (np.abs(cd - qd[:, 1:-1]).max(axis=1) <= slack).all(), (r, np.abs(cd - qd[:, 1:-1]).max(axis=1), slack)
        assert (np.abs(qd).max(axis=1) <= vmax * (1 + 8 * EPS)).all(), r
    record(test="rule: samples", case=name, rows=n, N=N, M=M, period=period, q_abs_err=err_q, qd_abs_err=err_v, largest_error_over_gate=ratio,
           bit_for_bit=bool(exact_s), counts_equal=True)


def on_the_polyline(x, q, segment, r):
    """every sample is x_i + s d_i with 0 <= s <= 1 on the rule's segment i or a neighbour (a waypoint belongs to both), and i + s never
    decreases.  Allowance: the interpolation's own rounding, a few ulps of the largest joint value, seen through the segment's length."""
    N, big = x.shape[1], np.abs(x).max()
    last = -1.0
    for k in range(q.shape[1]):
        best = None
        for i in range(max(int(segment[k]) - 1, 0), min(int(segment[k]) + 2, N - 1)):
            d = x[:, i + 1] - x[:, i]
            dd = float(d @ d)
            if dd == 0.0:
                continue
            s = float((q[:, k] - x[:, i]) @ d) / dd
            res = float(np.abs(q[:, k] - (x[:, i] + s * d)).max())
            tol = 16 * EPS * big / math.sqrt(dd)
            if res <= 16 * EPS * big and -tol <= s <= 1 + tol and (best is None or res < best[0]):
                best = (res, i + min(max(s, 0.0), 1.0), tol)
        if best is None:  # (a row that does not move: every sample is the goal = every waypoint)
            assert np.array_equal(q[:, k], x[:, N - 1]), (r, k)
            continue
        assert best[1] >= last - 2 * best[2], (r, k, best, last)
        last = max(last, best[1])


def raw_sample(ctx, X, prof, rows, period, M, n=None, N=None, spare=1, drop=None):
    """the C entry point with output buffers of `spare` slots more than the call may write, filled with sentinels -> (rc, message, q, qd, count)"""
    lib = ctx.lib
    Xd = ctx.to_dev(np.asarray(X), torch.float64)
    pd = {k: ctx.to_dev(np.asarray(prof[k]), torch.float64) for k in ("y", "phase", "times", "duration", "seg")}
    listed = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32))
    Rn = (X.shape[0] if listed is None else len(listed)) + spare
    Mb = max(min(M, 4096), 1)
    with torch.cuda.stream(ctx.stream):
        q = torch.full((Rn, 7, Mb), -5.0, dtype=torch.float64, device=ctx.device)
        qd = torch.full((Rn, 7, Mb), -6.0, dtype=torch.float64, device=ctx.device)
        cnt = torch.full((Rn,), -7, dtype=torch.int32, device=ctx.device)
    ctx.sync()
    ptrs = {k: C.c_void_p(v.data_ptr()) for k, v in pd.items()}
    if drop:
        ptrs[drop] = None
    rc = lib.edmp_sample_rows_dev(ctx.h, C.c_void_p(Xd.data_ptr()), X.shape[0] if n is None else n, X.shape[2] if N is None else N, ptrs["y"], ptrs["phase"],
                                  ptrs["times"], ptrs["duration"], ptrs["seg"], None if listed is None else _capi.as_pi32(listed), 0 if listed is None else len(listed),
                                  float(period), int(M), C.c_void_p(q.data_ptr()), C.c_void_p(qd.data_ptr()), C.c_void_p(cnt.data_ptr()))
    msg = lib.edmp_last_error().decode() if rc else ""
    ctx.sync()
    return rc, msg, ctx.to_host(q), ctx.to_host(qd), ctx.to_host(cnt)


@pytest.mark.parametrize("M", [1, 255, 256, 257, 1025])
def test_sample_chunk_edges(M):
    """M around the 256-sample chunk: the same bits as the first M samples of a longer call, nothing written past sample M - 1 or past the
    listed slots, and count is the row's true count whatever M"""
    from edmp_amd.runtime import get_context

    ctx = get_context(DEV)
    c = I.case("coarse_N4_n4_big_jump")
    prof = E.time_rows(c["X"], *c["limits"], device=DEV)
    period = float(np.max(prof["duration"])) / 1100.5
    full = E.sample_rows(c["X"], prof, period, max_samples=1400, device=DEV)
    assert full["count"].max() == 1102 and full["count"].min() > 257
    rc, msg, q, qd, cnt = raw_sample(ctx, c["X"], prof, None, period, M)
    assert rc == 0, msg
    assert np.array_equal(bits(q[:4]), bits(full["q"][:, :, :M])) and np.array_equal(bits(qd[:4]), bits(full["qd"][:, :, :M])) and np.array_equal(cnt[:4], full["count"])
    assert (q[4] == -5.0).all() and (qd[4] == -6.0).all() and cnt[4] == -7
    smp = I.sample_row(c["X"][2], c["ref"]["rows"][2], period, M)
    gate = c["limits"][0] * 4 * 25 * EPS * c["ref"]["duration"][2] + 64 * EPS * np.abs(c["X"][2]).max()
    assert (np.abs(q[2] - smp["q"]).max(axis=1) <= gate).all()


def test_a_scrambled_row_list_fills_its_slots_and_nothing_else():
    """rows = [7, 2, 5] of nine: slot k holds row rows[k]'s samples, bit for bit those of the call over every row; the slots behind the list
    keep their sentinels; the Python call returns the same in list order"""
    from edmp_amd.runtime import get_context

    ctx = get_context(DEV)
    c = I.case("walk_N50_n9")
    prof = E.time_rows(c["X"], *c["limits"], device=DEV)
    period = period_of(c["ref"], 520.5)
    full = E.sample_rows(c["X"], prof, period, device=DEV)
    M = full["q"].shape[2]
    rows = [7, 2, 5]
    rc, msg, q, qd, cnt = raw_sample(ctx, c["X"], prof, rows, period, M, spare=2)
    assert rc == 0, msg
    assert np.array_equal(bits(q[:3]), bits(full["q"][rows])) and np.array_equal(bits(qd[:3]), bits(full["qd"][rows])) and np.array_equal(cnt[:3], full["count"][rows])
    assert (q[3:] == -5.0).all() and (qd[3:] == -6.0).all() and (cnt[3:] == -7).all()
    sub = E.sample_rows(c["X"], prof, period, rows=rows, max_samples=M, device=DEV)
    assert same(sub, dict(q=full["q"][rows], qd=full["qd"][rows], count=full["count"][rows]), SAMPLES)
    short = int(full["count"][rows].max()) - 1
    with pytest.raises(ValueError, match=f"max_samples = {short} is smaller than the {short + 1} samples of row"):
        E.sample_rows(c["X"], prof, period, rows=rows, max_samples=short, device=DEV)
    assert E.sample_rows(c["X"], prof, period, rows=[2], device=DEV)["q"].shape == (1, 7, int(full["count"][2]))  # M defaults to the listed rows' largest count


def test_scene_batch_equals_serial_calls():
    """3 scenes x 5 rows in one launch: every profile array and every sample of scene s equals guides[s]'s own call on X[s], bit for bit,
    also with the state and the results on the device"""
    from edmp_amd.guide import SceneBatch

    guides = [make_guide(50 + s, 5, no)[0] for s, no in enumerate((1, 7, 16))]
    batch = SceneBatch(guides)
    X = I.walk_rows(31, 15, 50).reshape(3, 5, 7, 50)
    serial = [g.time_rows(X[s]) for s, g in enumerate(guides)]
    got = batch.time_rows(X)
    assert got["y"].shape == (3, 5, 50) and got["phase"].shape == (3, 5, 49, 3) and got["duration"].shape == (3, 5) and got["limit"].shape == (3, 5, 50)
    for s in range(3):
        assert same({k: got[k][s] for k in PROFILE}, serial[s], PROFILE), s
    period = float(got["duration"].max()) / 200.5
    M = E.sample_count(got["duration"].max(), period)
    smp = batch.sample_rows(X, got, period, max_samples=M)
    assert smp["q"].shape == (15, 7, M)
    for s, g in enumerate(guides):
        one = g.sample_rows(X[s], serial[s], period, max_samples=M)
        assert same({k: smp[k][5 * s:5 * s + 5] for k in SAMPLES}, one, SAMPLES), s
    dev = batch.time_rows(torch.as_tensor(X, device=DEV), return_device=True)
    assert all(np.array_equal(bits(dev[k].cpu().numpy()), bits(got[k])) for k in PROFILE)
    sub = batch.sample_rows(torch.as_tensor(X, device=DEV), dev, period, rows=[11, 0], max_samples=M, return_device=True)
    assert np.array_equal(bits(sub["q"].cpu().numpy()), bits(smp["q"][[11, 0]])) and np.array_equal(sub["count"].cpu().numpy(), smp["count"][[11, 0]])


def test_a_segmented_run_goes_on(tiny_net):
    """a time_rows and a sample_rows call between two segments of a segmented run: the run's result is bit-identical to the uninterrupted one"""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = run_cfgs(101)
    s, gl = np.asarray(scenes.DEFAULT_START, dtype=np.float64), np.asarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    rs = np.random.RandomState(11)
    g = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, cfgs["total_batch_size"])
    c = I.case("walk_N50_n9")

    def between():  # (called once, after the noise of both segments has been drawn from rs)
        prof = g.time_rows(c["X"])
        return prof, g.sample_rows(c["X"], prof, 0.05, rows=[8, 1])

    prof, smp = segmented_run_goes_on(tiny_net, g, cfgs, s, gl, rs, between)
    assert np.array_equal(prof["limit"], c["ref"]["limit"]) and smp["count"].tolist() == [I.sample_count(c["ref"]["duration"][r], 0.05) for r in (8, 1)]


def raw_time(ctx, X, limits, n=None, N=None, drop=None):
    """edmp_time_rows_dev with sentinel-filled outputs -> (rc, message, dict of host arrays)"""
    lib = ctx.lib
    Xd = ctx.to_dev(np.asarray(X), torch.float64)
    n0, _, N0 = X.shape
    with torch.cuda.stream(ctx.stream):
        out = dict(y=torch.full((n0, N0), -5.0, dtype=torch.float64, device=ctx.device), phase=torch.full((n0, N0 - 1, 3), -5.0, dtype=torch.float64, device=ctx.device),
                   times=torch.full((n0, N0), -5.0, dtype=torch.float64, device=ctx.device), duration=torch.full((n0,), -5.0, dtype=torch.float64, device=ctx.device),
                   limit=torch.full((n0, N0), -7, dtype=torch.int32, device=ctx.device), seg=torch.full((n0, N0 - 1, 2), -5.0, dtype=torch.float64, device=ctx.device))
    ctx.sync()
    lim = [np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in limits]
    ptrs = [None if k == drop else C.c_void_p(out[k].data_ptr()) for k in PROFILE]
    rc = lib.edmp_time_rows_dev(ctx.h, C.c_void_p(Xd.data_ptr()), n0 if n is None else n, N0 if N is None else N, *(_capi.as_pd(v) for v in lim), *ptrs)
    msg = lib.edmp_last_error().decode() if rc else ""
    ctx.sync()
    return rc, msg, {k: ctx.to_host(v) for k, v in out.items()}


def test_refusals():
    """each bad argument is refused with a message that names the entry point and the value; the outputs keep their sentinels and a
    following call gives what it gave before"""
    from edmp_amd.runtime import get_context

    ctx = get_context(DEV)
    c = I.case("coarse_N4_n4_big_jump")
    X, lim = c["X"], c["limits"]
    before = E.time_rows(X, *lim, device=DEV)
    period = float(before["duration"].max()) / 40.5
    smp_before = E.sample_rows(X, before, period, device=DEV)

    def limits(which, j, v):
        out = [np.array(a) for a in lim]
        out[which][j] = v
        return out

    bad_time = (("n = 0", dict(n=0), "n >= 1"), ("N = 1", dict(N=1), "(got 1)"), ("N = 65", dict(N=65), "(got 65)"), ("no limit buffer", dict(drop="limit"), "null pointer"),
                ("vmax[3] = 0", dict(limits=limits(0, 3, 0.0)), "vmax[3] = 0"), ("amax[6] = -2", dict(limits=limits(1, 6, -2.0)), "amax[6] = -2"),
                ("jump[0] = nan", dict(limits=limits(2, 0, float("nan"))), "jump[0] = nan"), ("vmax[1] = inf", dict(limits=limits(0, 1, float("inf"))), "vmax[1] = inf"))
    for what, kw, needle in bad_time:
        rc, msg, out = raw_time(ctx, X, kw.pop("limits", lim), **kw)
        assert rc == -1 and msg.startswith("edmp_time_rows_dev") and needle in msg, (what, rc, msg)
        assert all((out[k] == (-7 if k == "limit" else -5.0)).all() for k in PROFILE), what
    bad_sample = (("period = 0", dict(period=0.0), "period 0"), ("period = -1", dict(period=-1.0), "period -1"), ("period = nan", dict(period=float("nan")), "period nan"),
                  ("period = inf", dict(period=float("inf")), "period inf"), ("M = 0", dict(M=0), "M = 0"), ("M over the cap", dict(M=_capi.MAX_TIMED_SAMPLES + 1), f"M = {_capi.MAX_TIMED_SAMPLES + 1}"),
                  ("row 4 of 4", dict(rows=[0, 4]), "rows[1] = 4"), ("row -1", dict(rows=[-1]), "rows[0] = -1"), ("a row twice", dict(rows=[1, 0, 1]), "rows[2] = 1 is listed twice"),
                  ("more rows than there are", dict(rows=[0, 1, 2, 3, 0]), "5 listed rows"), ("n = 0", dict(n=0), "n >= 1"), ("N = 65", dict(N=65), "(got 65)"),
                  ("no duration", dict(drop="duration"), "null pointer"))
    for what, kw, needle in bad_sample:
        args = dict(rows=None, period=period, M=64)
        args.update(kw)
        rc, msg, q, qd, cnt = raw_sample(ctx, X, before, args.pop("rows"), args.pop("period"), args.pop("M"), **args)
        assert rc == -1 and msg.startswith("edmp_sample_rows_dev") and needle in msg, (what, rc, msg)
        assert (q == -5.0).all() and (qd == -6.0).all() and (cnt == -7).all(), what
    assert same(E.time_rows(X, *lim, device=DEV), before, PROFILE) and same(E.sample_rows(X, before, period, device=DEV), smp_before, SAMPLES)
    rc, msg, out = raw_time(ctx, X, lim)  # the accepted raw call writes what the Python call returns
    assert rc == 0 and same(out, before, PROFILE), msg
    for bad in (dict(trajectories=X[0]), dict(trajectories=X[:, :6])):
        with pytest.raises(ValueError, match="trajectories must be"):
            E.time_rows(bad["trajectories"], device=DEV)
    with pytest.raises(ValueError, match="profile\\['y'\\] must be"):
        E.sample_rows(X[:2], before, period, device=DEV)


def test_prefer_fastest_picks_the_row_the_rule_names():
    """select_row / choose_best_trajectory / select_rows with prefer="fastest": among the rows inside the trust region, the one whose timed
    motion at the default limits is the shortest under the host rule (the runner-up is 1e-6 s or more behind: no rounding decides)"""
    from edmp_amd.guide import SceneBatch

    parts = [make_guide(60 + s, 5, 3) for s in range(3)]
    X = I.walk_rows(33, 15, 50).reshape(3, 5, 7, 50).copy()
    starts, goals = np.stack([p[1]["start"] for p in parts]), np.stack([p[1]["goal"] for p in parts])
    dur = I.time_rows(X.reshape(15, 7, 50), *I.LIMITS)["duration"].reshape(3, 5)
    for s, (g, inp) in enumerate(parts):
        idx, vols, met = g.select_row(inp["start"], inp["goal"], X[s], prefer="fastest", volume_trust_region=1e9)
        order = np.argsort(dur[s])
        assert dur[s][order[1]] - dur[s][order[0]] > 1e-6
        assert idx == order[0] and vols.shape == (5,) and set(met) == set(E.METRIC_KEYS)
        assert np.array_equal(g.choose_best_trajectory(inp["start"], inp["goal"], X[s], prefer="fastest", volume_trust_region=1e9), X[s][order[0]])
        tight = g.select_row(inp["start"], inp["goal"], X[s], prefer="fastest", volume_trust_region=0.0)[0]
        assert tight == g.select_row(inp["start"], inp["goal"], X[s])[0]  # an empty trust region leaves the arg-min of the volume
    idx, _, _ = SceneBatch([p[0] for p in parts]).select_rows(starts, goals, X, prefer="fastest", volume_trust_region=1e9)
    assert idx.tolist() == np.argmin(dur, axis=1).tolist()
    with pytest.raises(ValueError, match="'fastest'"):
        parts[0][0].select_row(starts[0], goals[0], X[0], prefer="quickest")


def test_driver_times_the_chosen_plan():
    """infer_serial time_plan: off, no key is added and the results are the run's without it; True adds duration_s and the census of the
    chosen plan - the host rule's values for that trajectory; a period adds the sample count; the scene-group path reports the same"""
    import os

    import infer_serial
    from edmp_amd import scenes

    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "cfg_c1_plumbing.yaml")

    def run(k, **kw):
        np.random.seed(31)
        ds = scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=2, n_obstacles=6, n_cylinders=1)
        return infer_serial.run(cfg, dataset=ds, verbose=False, scenes_per_launch=k, **kw)

    off, on, group = run(1), run(1, time_plan=True), run(2, time_plan=0.01)
    keys = ("duration_s", "binding_constraints", "time_period_s", "timed_samples")
    for o, a, b in zip(off, on, group):
        assert not any(k in o for k in keys) and set(a) - set(o) == set(keys[:2]) and set(b) - set(o) == set(keys) | {"scenes_in_launch"}
        assert o["best_row"] == a["best_row"] == b["best_row"] and np.array_equal(o["trajectory"], a["trajectory"]) and np.array_equal(o["trajectory"], b["trajectory"])
        ref = I.time_row(a["trajectory"], *I.LIMITS)
        assert abs(a["duration_s"] - ref["duration"]) <= 4 * (3 * 49 + 16) * EPS * ref["duration"] and b["duration_s"] == a["duration_s"]
        assert a["binding_constraints"] == b["binding_constraints"] and sum(a["binding_constraints"].values()) == a["trajectory"].shape[1]
        assert b["timed_samples"] == I.sample_count(b["duration_s"], 0.01) and b["time_period_s"] == 0.01
    fast = run(1, prefer="fastest", time_plan=True)
    assert all(f["prefer"] == "fastest" and np.isfinite(f["duration_s"]) for f in fast)
    with pytest.raises(ValueError):
        infer_serial.run(cfg, verbose=False, time_plan=-0.5)
