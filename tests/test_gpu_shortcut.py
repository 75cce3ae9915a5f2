"""The shortcut stage (shortcut_rows_kernel, edmp_shortcut_rows_dev, edmp_scenes_shortcut_rows_dev) on the GPU against the rule of
tests/shortcut_inputs.py on admitted cases, against the GPU's own success_rows as the judge, and against itself where the property is
bit-equality.

On an admitted case (no decision of the rule sits on a rounding) spans, accepted and tested are compared exactly.  Trajectories and lengths
are compared under a gate of 4 x a yardstick: the deviation of the rule from itself with the piece interpolated the other way
((1 - g) x_i + g x_j) in float64 on the same inputs, with a floor of one ulp of the largest joint value (trajectories) / of the largest
length (lengths) - what the number type itself costs, with this project's margin of 4.  Every comparison prints its error, yardstick and
gate; with EDMP_SHORTCUT_PARITY_OUT=<file> the records are written there as JSON (profiles/shortcut_parity.json comes from such a run)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from edmp_amd import franka
from tests import repair_inputs as RI
from tests import sdf_reference as R
from tests import shortcut_inputs as I
from tests.sdf_gpu import DEV, recorder, run_cfgs, tiny_net  # noqa: F401  (tiny_net: this module's fixture)
from tests.sdf_term_suite import segmented_run_goes_on

pytestmark = pytest.mark.gpu
record, _write_records = recorder("shortcut parity", "EDMP_SHORTCUT_PARITY_OUT",
                                  "4 x the deviation of the host rule from itself with the piece interpolated the other way, floor one ulp of the largest "
                                  "joint value (trajectories) / of the largest length (lengths); spans, accepted and tested exactly")
KEYS = ("trajectories", "accepted", "tested", "length0", "length", "spans")
GATE = 4.0


def make_guide(case, device=DEV, **kw):
    """the guide of a case: its obstacles and kinds and the placeholder link boxes (shortcut_inputs.EXTENTS); the stage reads no row array"""
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = case["cfgs"]
    return IntersectionVolumeGuide(case["obstacle_config"], device, cfgs, cfgs["total_batch_size"], link_mesh_extents=franka.PLACEHOLDER_LINK_EXTENTS,
                                   obstacle_kinds=case["kinds"], **kw)


def bits(a):
    """raw bits, NaN patterns included"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same(a, b, keys=KEYS):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def zigzag_case(N=14, n=3, shift=0.0):
    """n zigzag rows on a graze scene: rows with accepted and rejected candidates (not necessarily admitted: for the bit-for-bit tests)"""
    g = RI.graze_scene(shift)
    return dict(g, X=I.zigzag_rows(g["start"], g["goal"], N, n), cfgs=RI.plain_cfgs(n))


@pytest.mark.parametrize("name", list(I.CASES))
def test_against_the_rule(name):
    """spans, accepted and tested equal the rule's exactly; trajectories and lengths within 4 x the yardstick; the ends keep their bits"""
    case = I.case(name)
    ref, y = case["ref"], case["yardstick"]
    out = make_guide(case).shortcut_rows(case["X"], passes=case["passes"], substeps=case["K"])
    err_x = float(np.abs(out["trajectories"] - ref["trajectories"]).max())
    err_l = float(max(np.abs(out["length"] - ref["length"]).max(), np.abs(out["length0"] - ref["length0"]).max()))
    record(test="rule", case=name, accepted=out["accepted"].tolist(), tested=out["tested"].tolist(), trajectory_abs_err=err_x, trajectory_yardstick=y["trajectories"],
           trajectory_ratio=err_x / y["trajectories"], length_abs_err=err_l, length_yardstick=y["length"], length_ratio=err_l / y["length"], gate=GATE)
    assert out["accepted"].dtype == np.int32 and out["tested"].dtype == np.int32 and out["spans"].dtype == np.int32 and out["spans"].shape == ref["spans"].shape
    assert np.array_equal(out["spans"], ref["spans"]), (out["spans"][:, :4].tolist(), ref["spans"][:, :4].tolist())
    assert np.array_equal(out["accepted"], ref["accepted"]) and np.array_equal(out["tested"], ref["tested"])
    assert np.array_equal(bits(out["trajectories"][:, :, [0, -1]]), bits(case["X"][:, :, [0, -1]]))
    assert err_x <= GATE * y["trajectories"], (err_x, y["trajectories"])
    assert err_l <= GATE * y["length"], (err_l, y["length"])


def test_log_cap():
    """the log holds the first log_cap spans, the counts stay true; log_cap = 0 gives an empty log"""
    case = I.case("N14_graze_zigzag")
    guide, ref = make_guide(case), case["ref"]
    out = guide.shortcut_rows(case["X"], passes=case["passes"], substeps=case["K"], log_cap=5)
    assert out["spans"].shape == (1, 5, 2) and np.array_equal(out["spans"], ref["spans"][:, :5]) and out["accepted"][0] == ref["accepted"][0] > 5
    none = guide.shortcut_rows(case["X"], passes=case["passes"], substeps=case["K"], log_cap=0)
    assert none["spans"].shape == (1, 0, 2) and same(none, out, ("trajectories", "accepted", "tested", "length0", "length"))


def test_property_free_rows_stay_free():
    """32 random plan-like rows whose straight line collides, judged by the GPU's own success_rows: every row free before is free after, no
    length grows, `within` is unchanged; always out of place.  (shortcut_inputs.check_property_seed holds the conditions on the inputs: at
    least 8 rows free and 8 colliding, at least half of the rows with a rejected candidate under the rule.)"""
    p = I.property_case()
    K, passes = I.PROPERTY["K"], I.PROPERTY["passes"]
    guide = make_guide(p)
    Xd = torch.as_tensor(p["X"], device=DEV)
    keep = Xd.clone()
    before = guide.success_rows(p["X"], substeps=K)
    assert np.array_equal(before["collision_free"], p["free"]) and p["free"].sum() >= 8 and (~p["free"]).sum() >= 8
    out = guide.shortcut_rows(Xd, passes=passes, substeps=K)
    assert torch.equal(Xd, keep)
    after = guide.success_rows(out["trajectories"], substeps=K)
    record(test="property", rows=int(p["free"].size), free_before=int(before["rows_collision_free"]), free_after=int(after["rows_collision_free"]),
           accepted=int(out["accepted"].sum()), tested=int(out["tested"].sum()), rows_with_a_rejection=int((out["tested"] > out["accepted"]).sum()))
    assert after["collision_free"][before["collision_free"]].all()
    assert (out["length"] <= out["length0"]).all() and (out["accepted"] >= 0).all()
    assert before["within"].all() and np.array_equal(after["within"], before["within"])  # (the rows start inside the limits: nothing can get better either)


@pytest.mark.parametrize("N,K", [(14, 4), (64, 8)])
def test_n_passes_in_one_launch_equal_n_launches(N, K):
    """passes = 3 in one launch = three launches of passes = 1, bit for bit - stale LDS or a misplaced barrier across passes would show"""
    case = zigzag_case(N)
    guide = make_guide(case)
    one = guide.shortcut_rows(case["X"], passes=3, substeps=K)
    X, acc, tst = case["X"], 0, 0
    for _ in range(3):
        step = guide.shortcut_rows(X, passes=1, substeps=K)
        X, acc, tst = step["trajectories"], acc + step["accepted"], tst + step["tested"]
        assert (step["accepted"] > 0).all()  # (every pass of these rows accepts: the one launch does not stop early)
    assert same(one, step, ("trajectories", "length")) and np.array_equal(one["accepted"], acc) and np.array_equal(one["tested"], tst)
    assert (one["tested"] > one["accepted"]).all() and not np.array_equal(one["trajectories"], case["X"])


def test_rows_subset():
    """rows= in non-monotonic order: the listed rows equal their values from the all-rows call, the others keep their bits and report 0 / NaN;
    the same row content at another row index gives the same bits"""
    case = zigzag_case(14, 3)
    guide = make_guide(case)
    full = guide.shortcut_rows(case["X"], passes=2)
    part = guide.shortcut_rows(case["X"], passes=2, rows=[2, 0])
    for k in KEYS:
        assert np.array_equal(bits(part[k][[2, 0]]), bits(full[k][[2, 0]])), k
    assert np.array_equal(bits(part["trajectories"][1]), bits(case["X"][1])) and part["accepted"][1] == 0 and part["tested"][1] == 0
    assert np.isnan(part["length0"][1]) and np.isnan(part["length"][1]) and (part["spans"][1] == -1).all()
    perm = [1, 2, 0]
    moved = guide.shortcut_rows(np.ascontiguousarray(case["X"][perm]), passes=2)
    for k in KEYS:
        assert np.array_equal(bits(moved[k]), bits(full[k][perm])), k
    assert (full["accepted"] > 0).all()


def test_clear_straight_row_and_report_only():
    """a straight row far from every obstacle keeps its bits with accepted = 0; passes = 0 is a pure report; a NaN row is untouched"""
    far = R.make_case(0, 1, 12, 7, 2, far=True)
    X, _ = I.line_state(far["start"], far["goal"], 14)
    out = make_guide(dict(far, cfgs=RI.plain_cfgs(1))).shortcut_rows(X, passes=2)
    assert np.array_equal(bits(out["trajectories"]), bits(X)) and out["accepted"][0] == 0 and out["tested"][0] == 0
    assert np.array_equal(bits(out["length"]), bits(out["length0"])) and abs(out["length0"][0] - I.path_length(X[0])) <= 4 * np.spacing(out["length0"][0])
    case = zigzag_case(14, 3)
    guide = make_guide(case)
    rep = guide.shortcut_rows(case["X"], passes=0)
    assert np.array_equal(bits(rep["trajectories"]), bits(case["X"])) and not rep["accepted"].any() and not rep["tested"].any() and (rep["spans"] == -1).all()
    assert np.array_equal(bits(rep["length"]), bits(rep["length0"])) and np.array_equal(bits(rep["length0"]), bits(guide.shortcut_rows(case["X"], passes=1)["length0"]))
    full = guide.shortcut_rows(case["X"], passes=2)
    for bad in (np.nan, np.inf):
        Xb = case["X"].copy()
        Xb[1, 3, 0] = bad  # (a pinned column counts: any element)
        out = guide.shortcut_rows(Xb, passes=2)
        assert out["accepted"].tolist() == [full["accepted"][0], -1, full["accepted"][2]] and out["tested"][1] == 0
        assert np.array_equal(bits(out["trajectories"][1]), bits(Xb[1])) and np.isnan(out["length0"][1]) and np.isnan(out["length"][1]) and (out["spans"][1] == -1).all()
        for k in KEYS:
            assert np.array_equal(bits(out[k][[0, 2]]), bits(full[k][[0, 2]])), k


def test_scene_batch_equals_serial_runs():
    """three scenes with 1, 7 (2 cylinders) and 64 obstacles, 2 rows each: every output of scene s equals guides[s].shortcut_rows(X[s]), bit
    for bit, also with the scenes in reversed order and with the state and the results on the device"""
    from edmp_amd.guide import SceneBatch

    parts = [zigzag_case(14, 2)]
    for seed, (no, ncyl) in ((41, (7, 2)), (42, (64, 0))):
        inp = R.make_case(seed, 2, 12, no, ncyl)
        parts.append(dict(inp, X=I.zigzag_rows(inp["start"], inp["goal"], 14, 2), cfgs=RI.plain_cfgs(2)))
    kw = dict(passes=2, substeps=4, log_cap=16)
    for order in ((0, 1, 2), (2, 1, 0)):
        ps = [parts[i] for i in order]
        guides = [make_guide(p) for p in ps]
        serial = [g.shortcut_rows(p["X"], **kw) for g, p in zip(guides, ps)]
        batch = SceneBatch(guides)
        X = np.stack([p["X"] for p in ps])
        got = batch.shortcut_rows(X, **kw)
        assert got["trajectories"].shape == (3, 2, 7, 14) and got["accepted"].shape == (3, 2) and got["spans"].shape == (3, 2, 16, 2)
        for s in range(3):
            for k in KEYS:
                assert np.array_equal(bits(got[k][s]), bits(serial[s][k])), (order, s, k)
        assert any(o["accepted"].any() for o in serial) and any((o["tested"] > o["accepted"]).any() for o in serial)
        Xd = torch.as_tensor(X, device=DEV)
        dev = batch.shortcut_rows(Xd, return_device=True, **kw)
        assert all(np.array_equal(bits(dev[k].cpu().numpy()), bits(got[k])) for k in KEYS) and np.array_equal(bits(Xd.cpu().numpy()), bits(X))
        sub = batch.shortcut_rows(X, rows=[5, 0], **kw)  # (rows index the S*B rows scene after scene)
        assert np.array_equal(bits(sub["trajectories"][2, 1]), bits(got["trajectories"][2, 1])) and np.array_equal(bits(sub["trajectories"][1]), bits(X[1]))


def raw_call(guide, Xd, rows=None, n=None, N=None, K=4, passes=1, min_gain=1e-6, log_cap=4, name="edmp_shortcut_rows_dev", lead=None, spans=True):
    """the C entry point on a device state, with report buffers that a refused call must leave as they are -> (rc, message, counts, lengths, spans)"""
    from edmp_amd import _capi
    from edmp_amd.runtime import ptr

    ctx = guide.ctx
    n = Xd.shape[0] if n is None else n
    with torch.cuda.stream(ctx.stream):
        cnt = torch.full((2, Xd.shape[0]), -7, dtype=torch.int32, device=ctx.device)
        ln = torch.full((Xd.shape[0], 2), -5.0, dtype=torch.float64, device=ctx.device)
        sp = torch.full((Xd.shape[0], 4, 2), -9, dtype=torch.int32, device=ctx.device)
    lst = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32))
    lead = (n,) if lead is None else lead
    dh = np.ascontiguousarray(franka.dh_table_f64())
    rc = getattr(ctx.lib, name)(ctx.h, ptr(Xd), *lead, Xd.shape[2] if N is None else N, None if lst is None else _capi.as_pi32(lst), 0 if lst is None else len(lst), K,
                                passes, min_gain, _capi.as_pd(dh), C.c_void_p(cnt[0].data_ptr()), C.c_void_p(cnt[1].data_ptr()), ptr(ln), ptr(sp) if spans else None, log_cap)
    return rc, (ctx.lib.edmp_last_error() or b"").decode() if rc else "", ctx.to_host(cnt), ctx.to_host(ln), ctx.to_host(sp)


def test_refusals():
    """each bad argument, duplicate rows included, is refused with a message that names the entry point and the value; X, the report
    buffers and a following call are what they were"""
    from edmp_amd import _capi
    from edmp_amd.guide import SceneBatch

    case = zigzag_case(14, 3)
    guide = make_guide(case)
    before = guide.shortcut_rows(case["X"], passes=2, log_cap=4)
    Xd = guide.ctx.to_dev(case["X"], torch.float64)
    bad = (("N = 2", dict(N=2), "(got 2)"), ("N = 65", dict(N=65), "(got 65)"), ("K = 0", dict(K=0), "substeps 0"), ("K = 65", dict(K=65), "substeps 65"),
           ("passes = -1", dict(passes=-1), "passes -1"), ("passes = 1025", dict(passes=1025), "passes 1025"), ("NaN min_gain", dict(min_gain=float("nan")), "min_gain"),
           ("negative min_gain", dict(min_gain=-0.5), "min_gain -0.5"), ("inf min_gain", dict(min_gain=float("inf")), "min_gain inf"),
           ("row 3 of 3", dict(rows=[0, 3]), "rows[1] = 3"), ("row -1", dict(rows=[-1]), "rows[0] = -1"), ("a row twice", dict(rows=[1, 0, 1]), "rows[2] = 1 is listed twice"),
           ("more rows than there are", dict(rows=[0, 1, 2, 0]), "4 listed rows"), ("n = 0", dict(n=0), "n >= 1"), ("log_cap = -1", dict(log_cap=-1), "log_cap -1"),
           ("a log without a buffer", dict(spans=False), "log_cap 4"))
    for what, kw, needle in bad:
        rc, msg, cnt, ln, sp = raw_call(guide, Xd, **kw)
        assert rc == -1 and msg.startswith("edmp_shortcut_rows_dev") and needle in msg, (what, rc, msg)
        assert (cnt == -7).all() and (ln == -5.0).all() and (sp == -9).all(), what
    rc, msg, cnt, _, _ = raw_call(guide, Xd, name="edmp_scenes_shortcut_rows_dev", lead=(1, 3))  # the batch's entry point on a single-scene guide
    assert rc == -3 and msg.startswith("edmp_scenes_shortcut_rows_dev") and (cnt == -7).all(), (rc, msg)
    assert np.array_equal(bits(guide.ctx.to_host(Xd)), bits(case["X"]))
    assert same(guide.shortcut_rows(case["X"], passes=2, log_cap=4), before)
    # the accepted raw call works in place and writes the listed rows only
    rc, msg, cnt, ln, sp = raw_call(guide, Xd, rows=[2], passes=2)
    assert rc == 0, msg
    Xh = guide.ctx.to_host(Xd)
    assert np.array_equal(bits(Xh[2]), bits(before["trajectories"][2])) and np.array_equal(bits(Xh[:2]), bits(case["X"][:2]))
    assert cnt[0].tolist() == [-7, -7, before["accepted"][2]] and cnt[1].tolist() == [-7, -7, before["tested"][2]]
    assert ln[2].tolist() == [before["length0"][2], before["length"][2]] and (ln[:2] == -5.0).all()
    assert np.array_equal(sp[2], before["spans"][2]) and (sp[:2] == -9).all()
    with pytest.raises(ValueError):
        guide.shortcut_rows(np.zeros((3, 6, 4)))
    with pytest.raises(_capi.EdmpError, match="passes -2"):
        guide.shortcut_rows(case["X"], passes=-2)
    # the single-scene entry point on a bound batch of two scenes, and a batch call with the wrong scene count
    batch = SceneBatch([make_guide(case, bind=False), make_guide(case, bind=False)])
    batch._bind()
    X2 = batch.ctx.to_dev(np.concatenate([case["X"], case["X"]]), torch.float64)
    rc, msg, _, _, _ = raw_call(batch, X2)
    assert rc == -3 and msg.startswith("edmp_shortcut_rows_dev"), (rc, msg)
    rc, msg, _, _, _ = raw_call(batch, X2, name="edmp_scenes_shortcut_rows_dev", lead=(3, 2))
    assert rc == -1 and msg.startswith("edmp_scenes_shortcut_rows_dev"), (rc, msg)
    with pytest.raises(_capi.EdmpError, match="listed twice"):
        batch.shortcut_rows(np.stack([case["X"], case["X"]]), rows=[4, 4])


def test_a_segmented_run_goes_on(tiny_net):
    """a shortcut_rows call between two segments of a segmented run: the run's result is bit-identical to the uninterrupted one"""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = run_cfgs(101)
    s, gl = np.asarray(scenes.DEFAULT_START, dtype=np.float64), np.asarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    rs = np.random.RandomState(11)
    g = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, cfgs["total_batch_size"])

    def between():  # (called once, after the noise of both segments has been drawn from rs)
        return g.shortcut_rows(I.zigzag_rows(gl, s, 50, 5), passes=1, rows=[4, 1])

    mid = segmented_run_goes_on(tiny_net, g, cfgs, s, gl, rs, between)
    assert np.isfinite(mid["length"][[4, 1]]).all() and (mid["tested"][[4, 1]] > 0).all() and np.isnan(mid["length"][0])


def test_history():
    """the small call gives the same bits after an N = 64, 64-obstacle, K = 8 call on the same context as on a fresh one"""
    from edmp_amd.runtime import Context

    small = zigzag_case(14, 3)
    inp = R.make_case(7, 3, 62, 64, 0)
    big = dict(inp, X=I.zigzag_rows(inp["start"], inp["goal"], 64, 3), cfgs=RI.plain_cfgs(3))
    outs = []
    for history in (False, True):
        ctx = Context(0)
        try:
            if history:
                out = make_guide(big, device=ctx).shortcut_rows(big["X"], passes=2, substeps=8, rows=[2, 0, 1])
                assert (out["tested"] > 0).all()
            outs.append(make_guide(small, device=ctx).shortcut_rows(small["X"], passes=2, rows=[1, 2]))
        finally:
            ctx.close()
    assert same(outs[0], outs[1]) and outs[0]["accepted"][1:].all()
    assert same(outs[0], make_guide(small).shortcut_rows(small["X"], passes=2, rows=[1, 2]))


def test_driver_shortcuts_between_the_repair_and_the_selection():
    """infer_serial --shortcut: off, no key is added; on, the serial loop and the scene-group path (one launch) report the same rows and
    choose the same plan, whose pinned ends are the run's without the option and whose joint path is no longer"""
    import infer_serial
    from edmp_amd import scenes

    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "cfg_c1_plumbing.yaml")

    def run(k, shortcut):
        np.random.seed(31)
        ds = scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=2, n_obstacles=6, n_cylinders=1)
        return infer_serial.run(cfg, dataset=ds, verbose=False, scenes_per_launch=k, shortcut=shortcut)

    off, serial, group = run(1, 0), run(1, 2), run(2, 2)
    assert len(off) == len(serial) == len(group) == 2
    for o, a, b in zip(off, serial, group):
        assert "rows_shortcut" not in o and "shortcut_passes" not in o and "shortcut_s" not in o["timings"]
        assert a["shortcut_passes"] == 2 and 0 <= a["rows_shortcut"] <= a["rows"] and "shortcut_s" in a["timings"] and "shortcut_s" in b["timings"]
        assert (a["rows_shortcut"], a["best_row"]) == (b["rows_shortcut"], b["best_row"])
        assert np.array_equal(a["trajectory"], b["trajectory"]) and np.isfinite(a["trajectory"]).all()
        assert np.array_equal(a["trajectory"][:, [0, -1]], o["trajectory"][:, [0, -1]])
        print(f"[shortcut driver] joint path {o['path_length']['joint']:.3f} -> {a['path_length']['joint']:.3f}, rows shortened {a['rows_shortcut']}/{a['rows']}")
        # (not an invariant: the selection is by swept volume and may pick another row once the rows are shortened.  It holds on these two
        # seeded scenes, whose random-init rows are hundreds of radians long before the stage)
        assert a["path_length"]["joint"] <= o["path_length"]["joint"]
        assert a["rows_collision_free"] >= o["rows_collision_free"]  # (the invariant: a collision-free row stays collision-free)
    assert sum(a["rows_shortcut"] for a in serial) > 0
    assert "rows_shortcut" in infer_serial.job_summary(serial, shortcut=True) and "rows_shortcut" not in infer_serial.job_summary(off)
    with pytest.raises(ValueError):
        infer_serial.run(cfg, verbose=False, shortcut=-1)
