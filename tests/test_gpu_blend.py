"""The corner-blend stage (blend_rows_kernel in blend.hip, the blended time_rows_kernel and sample_rows_kernel in timing.hip; edmp_blend_rows_dev,
edmp_scenes_blend_rows_dev, edmp_time_blended_rows_dev, edmp_sample_blended_rows_dev) on the GPU against the rule of tests/blend_inputs.py
on admitted cases, and against itself or the unblended entry points where the property is bit-equality.

Gates: 4 R 2^-53 of the quantity's scale, R the roundings of its longest chain as tests/blend_inputs.py counts them (gates(N)):
  code, halved, tested, limit, count    exactly
  beta                 R = 4, of beta itself
  y                    R = 2 (N - 1) + 16, of the row's largest y
  phase, times, blend  R = 4 (N - 1) + 24, of the row's duration
  q                    vmax_j x (the time gate, in seconds) + 64 x 2^-53 max |x|: a time error moves a sample along the path by at most its
                       speed; the rest is the interpolation's own rounding
  qd                   amax_j x (the time gate) + 64 x 2^-53 vmax_j: the same argument one derivative up
Bit-for-bit agreement is expected; every comparison prints its error and gate and says whether it was in fact bit for bit; with
EDMP_BLEND_PARITY_OUT=<file> the records are written there as JSON (profiles/blend_parity.json comes from such a run)."""
import ctypes as C

import numpy as np
import pytest
import torch

from edmp_amd import _capi, franka
from edmp_amd import evaluation as E
from tests import blend_inputs as I
from tests import repair_inputs as RI
from tests import timing_inputs as TI
from tests.sdf_gpu import DEV, recorder, run_cfgs, tiny_net  # noqa: F401  (tiny_net: this module's fixture)
from tests.sdf_term_suite import segmented_run_goes_on

pytestmark = pytest.mark.gpu
record, _write_records = recorder("blend parity", "EDMP_BLEND_PARITY_OUT",
                                  "code, halved, tested, limit and count exactly; beta within 4 x 4 x 2^-53 of itself; y within 4 (2 (N - 1) + 16) 2^-53 of the row's "
                                  "largest y; phase, times and blend within 4 (4 (N - 1) + 24) 2^-53 of the row's duration; q within vmax_j x that time gate + 64 x "
                                  "2^-53 max |x|; qd within amax_j x that time gate + 64 x 2^-53 vmax_j")
EPS = 2.0 ** -53
PROFILE = E.BLENDED_PROFILE_KEYS
SAMPLES = ("q", "qd", "count")
BLEND = ("beta", "code", "halved", "tested")


def bits(a):
    """raw bits, NaN patterns included"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same(a, b, keys):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def make_guide(obstacle_config, kinds, n, **kw):
    """a guide over the given obstacles with n plain rows and the placeholder link boxes (blend_inputs.EXTENTS); the stage reads no row array"""
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = RI.plain_cfgs(n)
    return IntersectionVolumeGuide(obstacle_config, DEV, cfgs, cfgs["total_batch_size"], link_mesh_extents=franka.PLACEHOLDER_LINK_EXTENTS, obstacle_kinds=kinds, **kw)


def case_guide(c):
    return make_guide(c["obstacle_config"], c["kinds"], c["X"].shape[0])


@pytest.mark.parametrize("name", I.names())
def test_against_the_rule(name):
    """every case through the three kernels: code, halved, tested, limit and count exactly; beta, every profile value and every sample inside
    their gates; the first sample is the start at rest, the last and every held sample the goal's bits at rest; |qd| <= vmax"""
    c = I.case(name)
    X, ref, host = c["X"], c["ref"], c["prof"]
    vmax, amax, jump = c["limits"]
    n, _, N = X.shape
    R = I.gates(N)
    g = case_guide(c)
    out = g.blend_rows(X, **I.call_args(c))
    assert out["code"].dtype == np.int32 and out["beta"].shape == (n, N) and out["tested"].shape == (n,)
    assert np.array_equal(out["code"], ref["code"]) and np.array_equal(out["halved"], ref["halved"]) and np.array_equal(out["tested"], ref["tested"])
    timed = np.isfinite(host["duration"])
    assert np.isnan(out["beta"][~timed]).all() and np.isfinite(out["beta"][timed]).all()
    err_b = float(np.abs(out["beta"][timed] - ref["beta"][timed]).max()) if timed.any() else 0.0
    gate_b = 4 * R["beta"] * EPS * ref["beta"][timed] if timed.any() else np.zeros(1)
    record(test="rule: blends", case=name, rows=n, N=N, substeps=c["Kb"], halvings=c["H"], obstacles=int(len(c["kinds"])), blended=int((ref["code"] == 3).sum()),
           blocked=int((ref["code"] == 4).sum()), tested=int(ref["tested"].sum()), beta_abs_err=err_b, beta_gate=float(gate_b.max()),
           bit_for_bit=bool(np.array_equal(bits(out["beta"]), bits(ref["beta"]))), codes_equal=True)
    assert (np.abs(out["beta"][timed] - ref["beta"][timed]) <= gate_b).all()

    prof = g.time_blended_rows(X, out["beta"], vmax, amax, jump)
    assert prof["limit"].dtype == np.int32 and np.array_equal(prof["limit"], host["limit"]) and prof["times"].shape == (n, N, 2)
    for k in ("y", "phase", "times", "seg", "blend"):
        assert np.isnan(prof[k][~timed]).all() and np.isfinite(prof[k][timed]).all(), k
    assert np.array_equal(np.isnan(prof["duration"]), ~timed)
    ymax = np.array([np.max(host["y"][r]) if timed[r] else 0.0 for r in range(n)])
    dur = np.where(timed, host["duration"], 0.0)
    gate_y, gate_t = 4 * R["y"] * EPS * ymax, 4 * R["times"] * EPS * dur
    err_y = np.array([np.abs(prof["y"][r] - host["y"][r]).max() if timed[r] else 0.0 for r in range(n)])
    err_t = np.array([max(np.abs(prof["phase"][r] - host["phase"][r]).max(initial=0.0), np.abs(prof["times"][r] - host["times"][r]).max(),
                          np.abs(prof["blend"][r] - host["blend"][r]).max(), abs(prof["duration"][r] - host["duration"][r])) if timed[r] else 0.0 for r in range(n)])
    record(test="rule: profile", case=name, rows=n, N=N, y_abs_err=float(err_y.max()), y_gate=float(gate_y.max()), time_abs_err=float(err_t.max()),
           time_gate=float(gate_t.max()), bit_for_bit=bool(same(prof, host, PROFILE)), limits_equal=True)
    assert (err_y <= gate_y).all(), (err_y, gate_y)
    assert (err_t <= gate_t).all(), (err_t, gate_t)

    period = I.choose_period(host["rows"], 150.5)
    smp = g.sample_blended_rows(X, prof, period)
    counts = np.array([TI.sample_count(d, period) for d in host["duration"]], dtype=np.int32)
    M = max(1, int(counts.max()))
    assert smp["q"].shape == (n, 7, M) and smp["qd"].shape == (n, 7, M) and smp["count"].dtype == np.int32 and np.array_equal(smp["count"], counts)
    err_q = err_v = ratio = 0.0
    exact = True
    for r in range(n):
        q, qd = smp["q"][r], smp["qd"][r]
        if not timed[r]:
            assert np.isnan(q).all() and np.isnan(qd).all()
            continue
        want = I.sample_row(X[r], host["rows"][r], period, M)
        gq = vmax * gate_t[r] + 64 * EPS * np.abs(X[r]).max()
        gv = amax * gate_t[r] + 64 * EPS * vmax
        eq, ev = np.abs(q - want["q"]).max(axis=1), np.abs(qd - want["qd"]).max(axis=1)
        err_q, err_v, ratio = max(err_q, float(eq.max())), max(err_v, float(ev.max())), max(ratio, float((eq / gq).max()), float((ev / gv).max()))
        exact = exact and np.array_equal(bits(q), bits(want["q"])) and np.array_equal(bits(qd), bits(want["qd"]))
        assert (eq <= gq).all() and (ev <= gv).all(), (r, eq, gq, ev, gv)
        held = counts[r] - 1
        assert np.array_equal(bits(q[:, held:]), bits(np.repeat(X[r][:, N - 1:], M - held, axis=1))) and not qd[:, held:].any(), r
        assert np.array_equal(bits(q[:, 0]), bits(X[r][:, 0])) and not qd[:, 0].any(), r
        assert (np.abs(qd).max(axis=1) <= vmax * (1 + 8 * EPS)).all(), r
    record(test="rule: samples", case=name, rows=n, N=N, M=M, period=period, q_abs_err=err_q, qd_abs_err=err_v, largest_error_over_gate=ratio,
           bit_for_bit=bool(exact), counts_equal=True)


@pytest.mark.parametrize("name", TI.names())
def test_beta_zero_gives_the_unblended_entry_points_bits(name):
    """beta = 0 everywhere: y, phase, duration, limit and seg have edmp_time_rows_dev's bits, times[i] = (T_i, T_i), blend = 0 (NaN on a row that
    is not timed), and q, qd and count have edmp_sample_rows_dev's bits"""
    c = TI.case(name)
    X, lim = c["X"], c["limits"]
    old = E.time_rows(X, *lim, device=DEV)
    new = E.time_blended_rows(X, np.zeros((X.shape[0], X.shape[2])), *lim, device=DEV)
    assert same(new, old, ("y", "phase", "duration", "limit", "seg"))
    assert np.array_equal(bits(new["times"][:, :, 0]), bits(old["times"])) and np.array_equal(bits(new["times"][:, :, 1]), bits(old["times"]))
    timed = np.isfinite(old["duration"])
    assert not new["blend"][timed].any() and np.isnan(new["blend"][~timed]).all()
    d = np.nanmax(old["duration"])
    period = float(d) / 300.5 if d > 0 else 1e-3
    a, b = E.sample_blended_rows(X, new, period, device=DEV), E.sample_rows(X, old, period, device=DEV)
    assert a["q"].shape == b["q"].shape and same(a, b, SAMPLES) and np.array_equal(a["t"], b["t"])


def raw_blend(g, X, c, rows=None, name="edmp_blend_rows_dev", lead=None, N=None, spare=1, **kw):
    """the C entry point with sentinel-filled outputs of `spare` rows more than the state has -> (rc, message, beta, code, halved, tested)"""
    ctx, lib = g.ctx, g.ctx.lib
    Xd = ctx.to_dev(np.asarray(X), torch.float64)
    n, _, N0 = X.shape
    a = dict(I.call_args(c))
    a.update(kw)
    with torch.cuda.stream(ctx.stream):
        beta = torch.full((n + spare, N0), -5.0, dtype=torch.float64, device=ctx.device)
        code = torch.full((n + spare, N0), -7, dtype=torch.int32, device=ctx.device)
        halved = torch.full((n + spare, N0), -8, dtype=torch.int32, device=ctx.device)
        tested = torch.full((n + spare,), -9, dtype=torch.int32, device=ctx.device)
    ctx.sync()
    listed = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32))
    lim = [np.ascontiguousarray(np.asarray(a[k], dtype=np.float64)) for k in ("vmax", "amax", "jump")]
    dev = np.ascontiguousarray(np.broadcast_to(np.asarray(a["deviation"], dtype=np.float64), (7,)))
    dh = np.ascontiguousarray(franka.dh_table_f64())
    rc = getattr(lib, name)(ctx.h, C.c_void_p(Xd.data_ptr()), *((n,) if lead is None else lead), N0 if N is None else N, None if listed is None else _capi.as_pi32(listed),
                            0 if listed is None else len(listed), *(_capi.as_pd(v) for v in lim), _capi.as_pd(dev), float(a["reach"]), int(a["substeps"]),
                            int(a["halvings"]), _capi.as_pd(dh), *(C.c_void_p(t.data_ptr()) for t in (beta, code, halved, tested)))
    msg = lib.edmp_last_error().decode() if rc else ""
    ctx.sync()
    return rc, msg, ctx.to_host(beta), ctx.to_host(code), ctx.to_host(halved), ctx.to_host(tested)


def test_listed_rows_are_written_and_nothing_else():
    """rows = [7, 2, 5] of nine: the listed rows' entries are the full call's bits, every other entry keeps its sentinel; the Python call
    reports the others as unblended (beta 0, code 0); the sampler's slot k holds row rows[k], the slots behind the list keep their sentinels"""
    c = I.case("walk_N50_n9_o7c2")
    g, X, rows = case_guide(c), c["X"], [7, 2, 5]
    full = g.blend_rows(X, **I.call_args(c))
    g._bind()
    rc, msg, beta, code, halved, tested = raw_blend(g, X, c, rows)
    assert rc == 0, msg
    others = [r for r in range(10) if r not in rows]
    assert np.array_equal(bits(beta[rows]), bits(full["beta"][rows])) and np.array_equal(code[rows], full["code"][rows]) and np.array_equal(halved[rows], full["halved"][rows])
    assert np.array_equal(tested[rows], full["tested"][rows])
    assert (beta[others] == -5.0).all() and (code[others] == -7).all() and (halved[others] == -8).all() and (tested[others] == -9).all()
    sub = g.blend_rows(X, rows=rows, **I.call_args(c))
    assert same({k: sub[k][rows] for k in BLEND}, {k: full[k][rows] for k in BLEND}, BLEND)
    assert not sub["beta"][others[:-1]].any() and not sub["code"][others[:-1]].any() and not sub["tested"][others[:-1]].any()
    prof = g.time_blended_rows(X, full["beta"], *c["limits"])
    period = I.choose_period(c["prof"]["rows"], 520.5)
    whole = g.sample_blended_rows(X, prof, period)
    M = whole["q"].shape[2]
    part = g.sample_blended_rows(X, prof, period, rows=rows, max_samples=M)
    assert same(part, dict(q=whole["q"][rows], qd=whole["qd"][rows], count=whole["count"][rows]), SAMPLES)
    assert M > 512  # (three 256-sample chunks, the last one partial)
    with pytest.raises(_capi.EdmpError, match="listed twice"):
        g.blend_rows(X, rows=[1, 1], **I.call_args(c))


def test_scene_batch_equals_serial_calls():
    """3 scenes x 3 rows in one launch - 1, 7 and 64 obstacles, cylinders among them, each scene's own probe deciding its first row: every
    output of scene s equals guides[s]'s own call on X[s], bit for bit, through all three stages, also with the state on the device"""
    from edmp_amd.guide import SceneBatch

    scenes = [I.middle_probe(), I.with_far(*I.middle_probe(True), 7, 2), I.with_far(*I.end_probe(), 64, 8)]
    X = np.stack([np.concatenate([I.l_corner(), TI.coarse_rows(70 + s, 2, 3)]) for s in range(3)])
    kw = dict(deviation=I.L_DEVIATION, reach=0.4, substeps=4, halvings=2)
    guides = [make_guide(oc, kd, 3) for oc, kd in scenes]
    serial = [g.blend_rows(X[s], **kw) for s, g in enumerate(guides)]
    ref = [I.blend_rows(X[s], oc, kd, I.LIMITS, kw["deviation"], kw["reach"], kw["substeps"], kw["halvings"]) for s, (oc, kd) in enumerate(scenes)]
    batch = SceneBatch(guides)
    got = batch.blend_rows(X, **kw)
    assert got["beta"].shape == (3, 3, 3) and got["tested"].shape == (3, 3)
    for s in range(3):
        assert same({k: got[k][s] for k in BLEND}, serial[s], BLEND), s
        assert np.array_equal(serial[s]["code"], ref[s]["code"]) and np.array_equal(serial[s]["halved"], ref[s]["halved"]) and np.array_equal(serial[s]["tested"], ref[s]["tested"]), s
        assert serial[s]["code"][0, 1] == 3 and serial[s]["halved"][0, 1] == 1  # the scene's own probe was seen
    profs = [g.time_blended_rows(X[s], serial[s]["beta"]) for s, g in enumerate(guides)]
    prof = batch.time_blended_rows(X, got["beta"])
    assert prof["times"].shape == (3, 3, 3, 2) and prof["duration"].shape == (3, 3)
    for s in range(3):
        assert same({k: prof[k][s] for k in PROFILE}, profs[s], PROFILE), s
    period = float(prof["duration"].max()) / 200.5
    M = E.sample_count(prof["duration"].max(), period)
    smp = batch.sample_blended_rows(X, prof, period, max_samples=M)
    assert smp["q"].shape == (9, 7, M)
    for s, g in enumerate(guides):
        one = g.sample_blended_rows(X[s], profs[s], period, max_samples=M)
        assert same({k: smp[k][3 * s:3 * s + 3] for k in SAMPLES}, one, SAMPLES), s
    Xd = torch.as_tensor(X, device=DEV)
    dev = batch.blend_rows(Xd, return_device=True, **kw)
    assert all(np.array_equal(bits(dev[k].cpu().numpy()), bits(got[k])) for k in BLEND)
    dprof = batch.time_blended_rows(Xd, dev["beta"], return_device=True)
    assert all(np.array_equal(bits(dprof[k].cpu().numpy()), bits(prof[k])) for k in PROFILE)
    sub = batch.sample_blended_rows(Xd, dprof, period, rows=[7, 0], max_samples=M, return_device=True)
    assert np.array_equal(bits(sub["q"].cpu().numpy()), bits(smp["q"][[7, 0]])) and np.array_equal(sub["count"].cpu().numpy(), smp["count"][[7, 0]])


def test_a_segmented_run_goes_on(tiny_net):
    """the three calls between two segments of a segmented run: the run's result is bit-identical to the uninterrupted one"""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = run_cfgs(101)
    s, gl = np.asarray(scenes.DEFAULT_START, dtype=np.float64), np.asarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    rs = np.random.RandomState(11)
    g = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, cfgs["total_batch_size"])
    X = TI.walk_rows(11, 9, 50)

    def between():  # (called once, after the noise of both segments has been drawn from rs)
        bl = g.blend_rows(X, rows=[8, 1])
        prof = g.time_blended_rows(X, bl["beta"])
        return bl, prof, g.sample_blended_rows(X, prof, 0.05, rows=[8, 1])

    bl, prof, smp = segmented_run_goes_on(tiny_net, g, cfgs, s, gl, rs, between)
    assert (bl["tested"][[8, 1]] > 0).all() and not bl["tested"][[0, 2, 3, 4, 5, 6, 7]].any() and np.isfinite(prof["duration"]).all()
    assert smp["count"].tolist() == [E.sample_count(prof["duration"][r], 0.05) for r in (8, 1)]


def test_refusals():
    """each bad argument is refused with a message that names the entry point and the value; the outputs keep their sentinels and a following
    call gives what it gave before; a scene batch handed to the single-scene entry is refused, and a single-scene guide to the batch's"""
    from edmp_amd.guide import SceneBatch

    c = I.case("coarse_N4_n4_o1_K1")
    g, X = case_guide(c), c["X"]
    before = g.blend_rows(X, **I.call_args(c))
    g._bind()
    bad = (("reach = 0.46", dict(reach=0.46), "reach 0.46"), ("reach = 0", dict(reach=0.0), "reach 0"), ("reach = nan", dict(reach=float("nan")), "reach nan"),
           ("N = 65", dict(N=65), "(got 65)"), ("N = 1", dict(N=1), "(got 1)"), ("substeps = 0", dict(substeps=0), "substeps 0"), ("substeps = 9", dict(substeps=9), "substeps 9"),
           ("halvings = -1", dict(halvings=-1), "halvings -1"), ("halvings = 9", dict(halvings=9), "halvings 9"),
           ("deviation = 0", dict(deviation=0.0), "deviation[0] = 0"), ("deviation[3] = -1", dict(deviation=[0.01, 0.01, 0.01, -1.0, 0.01, 0.01, 0.01]), "deviation[3] = -1"),
           ("amax[6] = nan", dict(amax=[1, 1, 1, 1, 1, 1, float("nan")]), "amax[6] = nan"), ("row 4 of 4", dict(rows=[0, 4]), "rows[1] = 4"),
           ("a row twice", dict(rows=[1, 0, 1]), "rows[2] = 1 is listed twice"), ("n = 0", dict(lead=(0,)), "n >= 1"))
    for what, kw, needle in bad:
        rc, msg, beta, code, halved, tested = raw_blend(g, X, c, **kw)
        assert rc == -1 and msg.startswith("edmp_blend_rows_dev") and needle in msg, (what, rc, msg)
        assert (beta == -5.0).all() and (code == -7).all() and (halved == -8).all() and (tested == -9).all(), what
    assert same(g.blend_rows(X, **I.call_args(c)), before, BLEND)
    g._bind()
    rc, msg, beta, code, halved, tested = raw_blend(g, X, c)  # the accepted raw call writes what the Python call returns
    assert rc == 0 and same(dict(beta=beta[:4], code=code[:4], halved=halved[:4], tested=tested[:4]), before, BLEND), msg
    rc, msg, *_ = raw_blend(g, X, c, name="edmp_scenes_blend_rows_dev", lead=(1, 4))
    assert rc == -3 and msg.startswith("edmp_scenes_blend_rows_dev"), (rc, msg)
    batch = SceneBatch([make_guide(c["obstacle_config"], c["kinds"], 4, bind=False), make_guide(c["obstacle_config"], c["kinds"], 4, bind=False)])
    batch._bind()
    X2 = np.concatenate([X, X])
    rc, msg, *_ = raw_blend(batch, X2, c)
    assert rc == -3 and msg.startswith("edmp_blend_rows_dev") and "scene batch" in msg, (rc, msg)
    rc, msg, *_ = raw_blend(batch, X2, c, name="edmp_scenes_blend_rows_dev", lead=(3, 2))
    assert rc == -1 and msg.startswith("edmp_scenes_blend_rows_dev"), (rc, msg)
    two = batch.blend_rows(X2, **I.call_args(c))
    assert same({k: two[k][0] for k in BLEND}, before, BLEND) and same({k: two[k][1] for k in BLEND}, before, BLEND)
    # the timing and sampling entry points
    prof = E.time_blended_rows(X, before["beta"], *c["limits"], device=DEV)
    with pytest.raises(ValueError, match="beta must be"):
        E.time_blended_rows(X, before["beta"][:2], device=DEV)
    with pytest.raises(ValueError, match="profile\\['times'\\] must be"):
        E.sample_blended_rows(X, dict(prof, times=prof["times"][:, :, 0]), 0.01, device=DEV)
    with pytest.raises(_capi.EdmpError, match="edmp_time_blended_rows_dev.*got 65"):
        E.time_blended_rows(np.zeros((1, 7, 65)), np.zeros((1, 65)), device=DEV)
    with pytest.raises(ValueError, match="period must be"):
        E.sample_blended_rows(X, prof, 0.0, device=DEV)


def test_driver_blends_the_chosen_plan():
    """infer_serial blend: off, no key is added and the results are the run's without it; on, `blended_duration_s`, the census of the chosen
    plan's corner codes over its interior waypoints, the arguments used and - with a period - `sampled_motion`: the sample count is the
    faster motion's; the scene-group path reports the same values; blend without time_plan and a reach past 0.45 are refused.  (The numbers
    themselves are held to the rule by the tests above: this one is about the driver's plumbing.)"""
    import os

    import infer_serial
    from edmp_amd import scenes

    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "cfg_c1_plumbing.yaml")

    def run(k, **kw):
        np.random.seed(31)
        ds = scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=2, n_obstacles=6, n_cylinders=1)
        return infer_serial.run(cfg, dataset=ds, verbose=False, scenes_per_launch=k, **kw)

    off, on, group = run(1, time_plan=0.01), run(1, time_plan=0.01, blend=0.01), run(2, time_plan=0.01, blend=0.01, blend_reach=0.4)
    keys = {"blended_duration_s", "corner_codes", "blend_deviation_rad", "blend_reach", "sampled_motion"}
    for o, a, b in zip(off, on, group):
        assert not (keys & set(o)) and set(a) - set(o) == keys and set(b) - set(o) == keys | {"scenes_in_launch"}
        assert np.array_equal(o["trajectory"], a["trajectory"]) and np.array_equal(o["trajectory"], b["trajectory"]) and a["duration_s"] == o["duration_s"]
        assert a["blended_duration_s"] == b["blended_duration_s"] and a["corner_codes"] == b["corner_codes"]
        assert sum(a["corner_codes"].values()) == a["trajectory"].shape[1] - 2 and set(a["corner_codes"]) == set(E.BLEND_CODE_NAMES)
        fast = min(a["duration_s"], a["blended_duration_s"])
        assert a["sampled_motion"] == ("blended" if a["blended_duration_s"] < a["duration_s"] else "polyline") and a["timed_samples"] == E.sample_count(fast, 0.01)
        assert a["timed_samples"] == b["timed_samples"] and (a["sampled_motion"] == "blended" or a["timed_samples"] == o["timed_samples"])
    with pytest.raises(ValueError, match="blend needs time_plan"):
        infer_serial.run(cfg, verbose=False, blend=0.01)
    with pytest.raises(ValueError, match="blend_reach"):
        infer_serial.run(cfg, verbose=False, time_plan=True, blend=0.01, blend_reach=0.5)
