"""The tool-pose goal term of the sphere signed-distance guide (sdf_goal_kernel, sdf_goal_rows_kernel, edmp_sdf_set_goal,
edmp_sdf_goal_rows_dev) on the GPU against its float64 autograd checker (tests/sdf_goal_inputs.py).

Gates: sdf_reference.gate - max(4 x the deviation of the checker's own formula in CPU float32 from float64, 4 f32 ulps) - relative to
the largest element for cost and gradient; distance and angle absolute, max(4 x the float32 yardstick's absolute deviation, 4 f32 ulps
of the largest tool / target coordinate, resp. of pi).  Where the report's largest cost is itself below float32's resolution of one lane
term - a single row against its own pose, float64 cost 0 - that resolution is the cost's gate (check_report).  Every comparison prints its error, yardstick and gate; with
EDMP_SDF_GOAL_PARITY_OUT=<file> the records are written there as JSON (profiles/sdf_goal_parity.json comes from such a run).  The term
has no kink: no element is excluded from any comparison."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import scene_sdf_inputs as SI
from tests import sdf_goal_inputs as I
from tests import sdf_reference as R
from tests import sdf_term_suite as suite
from tests.sdf_gpu import DEV, build_guide, recorder, tiny_net  # noqa: F401  (tiny_net: this module's fixture)

pytestmark = pytest.mark.gpu
T, B = I.T, I.B
record, _write_records = recorder("sdf goal parity", "EDMP_SDF_GOAL_PARITY_OUT",
                                  "cost, gradient: max(4 x CPU-float32 deviation from float64, 4 f32 ulps), relative to the largest element; distance, angle: "
                                  "absolute, max(4 x CPU-float32 deviation, 4 f32 ulps of the largest coordinate / of pi)")
TERM = suite.Term("goal", I, guide=103, rows=I.GOAL_ROWS, report=lambda g, X, start, goal, t: g.sdf_goal_rows(X, t), gradient_yardstick=I.gradient_yardstick,
                  guide_kw=lambda case: dict(goal_target=case["target"]))


def report_inputs(L, n, seed=0):
    return R.make_case(seed, n, L, I.N_OBSTACLES, I.N_CYLINDERS)


def check_report(what, out, joints, target, tool, w, r, k, n):
    """a sdf_goal_rows dict against the checker, every row; prints and records the four figures"""
    ev = I.evaluate_goal(joints, target, tool, w, r, k, want_grad=False)
    y = I.report_yardstick(joints, target, tool, w, r, k, ev)
    scale = float(np.abs(ev["cost"]).max())
    errs = dict(cost=float(np.abs(out["cost"] - ev["cost"]).max()), distance=float(np.abs(out["distance"] - ev["distance"]).max()),
                angle=float(np.abs(out["angle"] - ev["angle"]).max()), min_distance=float(np.abs(out["min_distance"] - ev["min_distance"]).max()))
    # Where a row's target is its own pose (n = 1 against the exact pose) the float64 cost - the "largest element" - is itself 0 and a
    # gate relative to it asks for an exact zero.  Only there, with the largest element below float32's resolution of one lane term,
    # the gate is that resolution: a coordinate difference no finer than GATE_FLOOR x the largest coordinate (the distance's own floor),
    # 3 - tr no finer than GATE_FLOOR x 3.  Everywhere else it is sdf_reference.gate relative to the largest element and nothing more.
    L = np.shape(joints)[2]
    ramp = np.array([sum(max(0, c - L + int(kk)) / int(kk) for c in range(1, L + 1)) for kk in k])
    resolution = float(np.max(np.asarray(w) * ramp * (3 * (R.GATE_FLOOR * ev["coord_max"]) ** 2 + np.asarray(r) * 3 * R.GATE_FLOOR)))
    gates = dict(cost=max(R.gate(y["cost"]) * scale, resolution if scale < resolution else 0.0), distance=I.abs_gate(y["distance_abs"], ev["coord_max"]),
                 angle=I.abs_gate(y["angle_abs"], math.pi),
                 min_distance=I.abs_gate(y["min_distance_abs"], ev["coord_max"]))
    record(test="report", what=what, n=n, abs_err=errs, cost_scale=scale, cost_resolution=resolution, yardstick=y, gate_abs=gates)
    for key in errs:
        assert out[key].shape == (n,) and out[key].dtype == np.float64, key
        assert errs[key] <= gates[key], (what, key, errs[key], gates[key])
    return ev


# ---- 1. the report, every row -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("derived", [False, True], ids=["explicit", "derived"])
@pytest.mark.parametrize("L,tool", [(1, "custom"), (2, "flange"), (48, "custom"), (62, "flange")])
def test_report_of_every_row(L, tool, derived):
    """sdf_goal_rows for n in {1, 3, 4, 5, 12} bound rows (partial and full four-row workgroups) with the windows 1, 8, L, L + 5 dealt
    round the rows, against the exact pose of row 0's last column, a random pose and a pose ~pi away in rotation; explicit targets, and
    the same poses derived from a goal configuration (a gradient call hands the pair over)"""
    from edmp_amd import guide_cfg as GC

    tool = I.CUSTOM_TOOL if tool == "custom" else "flange"
    windows = (1, 8, L, L + 5)
    for n in (1, 3, 4, 5, 12):
        inp = report_inputs(L, n)
        dicts = []  # n SDF rows, each with its own goal weight, rotation (0 among them) and window
        for i in range(n):
            d = R.guide_dict("sdf", False, 0.0, 500 + i)
            d["hyperparameters"]["sdf"].update(goal_weight=0.5 + 0.25 * i, goal_rotation=(0.0, 0.05, 1.0)[i % 3], goal_window=int(windows[i % 4]))
            dicts.append(d)
        cfgs = GC.build_guide_cfgs(dicts, 1, T)
        w, r, k = I.goal_arrays(cfgs)
        case = dict(inp, cfgs=cfgs, tool=tool, spheres=None, custom=False)
        for kind in I.TARGET_KINDS:
            qg = I.goal_configuration(kind, inp["joints"], seed=L)
            if derived:
                guide, target = build_guide(case), I.pose_of(qg, tool)
                guide.get_gradient(inp["joints"], inp["start"], qg, 0)  # (the pair of a gradient call: the target is the pose of qg)
            else:
                given = I.random_pose(L) if kind == "random" else I.pose_of(qg, tool)
                guide = build_guide(case, goal_target=given)
                target = guide._goal_target
            out = guide.sdf_goal_rows(inp["joints"], 0)
            ev = check_report(f"L{L} n{n} {kind} {'derived' if derived else 'explicit'}", out, inp["joints"], target, tool, w, r, k, n)
            if kind == "exact":
                assert ev["distance"][0] <= 1e-12 and ev["angle"][0] <= 1e-7
            if kind == "pi":
                assert ev["angle"][0] > math.pi - 2e-3
            if n == 3 and kind == "random":  # rows that are not the bound ones: weight 1, rotation 1, window L
                big = report_inputs(L, 5, seed=1)
                check_report(f"L{L} unbound rows {'derived' if derived else 'explicit'}", guide.sdf_goal_rows(big["joints"], 0), big["joints"], target, tool,
                             np.ones(5), np.ones(5), np.full(5, L), 5)


# ---- 2. the gradient of a mixed ensemble ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(I.CASES))
def test_gradient_of_a_mixed_ensemble(name):
    """get_gradient on SDF + self + goal, SDF + goal, plain SDF, iv and sv rows, with and without grad_norm, the weighted rows {1, 6, 7,
    10}: against checker(obstacle + self + goal), the normalised one un-normalised by the device's own sum g^2; every other row that
    does not normalise BIT-identical to the same ensemble built without the goal keys"""
    suite.gradient_of_a_mixed_ensemble(TERM, record, name)
    # the sum g^2 is that of the final elements: on the ensemble in which no row normalises the returned gradient is the raw one
    suite.rowsq_is_the_sum_of_the_final_squares(TERM, record, name)


# ---- runs ------------------------------------------------------------------------------------------------------------------------------
def far_case(L=48, seed=0):
    """rows of 48 waypoints in a scene whose obstacles are >= 5 m away: no obstacle hinge is active at any margin"""
    inp = R.make_case(seed, B, L, I.N_OBSTACLES, I.N_CYLINDERS, far=True)
    return dict(inp, cfgs=I.mixed_cfgs(L), tool=I.CUSTOM_TOOL, spheres=None, custom=False, L=L)


def test_clipped_joints(tiny_net):
    """3. a guided step on a state far outside the joint limits: the device clips x_post before it takes the gradient, and the weighted
    rows without a self term (6, normalised, and 7) equal the checker - smoothness + goal, the obstacles are far - evaluated at the
    clipped joints"""
    from edmp_amd import franka
    from edmp_amd.diffusion import Diffusion, guided_step

    case = far_case()
    cfgs, tool = case["cfgs"], case["tool"]
    target = I.pose_of(I.goal_configuration("random", case["joints"], 7), tool)
    guide = build_guide(case, goal_target=target)
    dif, t = Diffusion(T, DEV), 6
    assert guided_step(t)
    lo, hi = franka.joint_limits()
    rs = np.random.RandomState(8)
    X = np.concatenate([case["start"].reshape(1, 7, 1).repeat(B, 0), 1.6 * case["joints"], case["goal"].reshape(1, 7, 1).repeat(B, 0)], axis=2)
    st = dif.denoise_step(tiny_net, guide, X, 0.1 * rs.standard_normal(X.shape), t, case["start"], case["goal"], cfgs["guidance_schedule"])
    xin = st["x_post"][:, :, 1:-1]
    out_of = (xin < lo[None, :, None]) | (xin > hi[None, :, None])
    assert out_of[[6, 7]].mean() > 0.05  # a fair share of the elements is clipped
    q = np.clip(xin, lo[None, :, None], hi[None, :, None])
    rows = [6, 7]
    sdf = R.evaluate(q, case["start"], case["goal"], case["obstacle_config"], case["kinds"], R.case_spheres("default"), cfgs["sdf_margin"][:, t - 1], cfgs["smoothness"])
    assert sdf["collision"][rows].max() == 0.0  # (far obstacles: the obstacle part is the smoothness pull alone)
    w, r, k = I.goal_arrays(cfgs)
    goal = I.evaluate_goal(q, target, tool, w, r, k)
    g32 = I.evaluate_goal(q, target, tool, w, r, k, dtype=torch.float32)
    s32 = R.evaluate(q, case["start"], case["goal"], case["obstacle_config"], case["kinds"], R.case_spheres("default"), cfgs["sdf_margin"][:, t - 1], cfgs["smoothness"],
                     dtype=torch.float32)
    ref = sdf["grad"][rows] + goal["grad"][rows]
    scale = float(np.abs(ref).max())
    y = float(np.abs(s32["grad"][rows] + g32["grad"][rows] - ref).max() / scale)
    unclipped = I.evaluate_goal(xin, target, tool, w, r, k)["grad"][rows]
    nrm = float(np.float32(math.sqrt(float(dif.ctx.to_host(dif.sumsq_tensor())[0]))))
    err = {}
    for i, row in enumerate(rows):
        raw = st["grad"][row] * nrm if cfgs["grad_norm"][row] else st["grad"][row]
        err[row] = float(np.abs(raw - ref[i]).max()) / scale
    record(test="clipping", t=t, clipped_share=float(out_of[rows].mean()), row_rel_err=err, yardstick=y, gate=R.gate(y),
           unclipped_rel_diff=float(np.abs(unclipped - goal["grad"][rows]).max() / scale))
    assert float(np.abs(unclipped - goal["grad"][rows]).max() / scale) > 100 * R.gate(y)  # clipping matters on these inputs
    for row in rows:
        assert err[row] <= R.gate(y), (row, err[row], y)


def loop_inputs(seed=21):
    """a (B, 7, 50) state at step 8 - noisy lines start -> goal - and the eight draws of the steps 8 .. 1"""
    from edmp_amd import scenes

    rs = np.random.RandomState(seed)
    a, b = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    s = np.linspace(0, 1, 50)
    X = (a[:, None] * (1 - s) + b[:, None] * s)[None] + 0.05 * rs.standard_normal((B, 7, 50))
    X[:, :, 0], X[:, :, -1] = a[None], b[None]
    return np.ascontiguousarray(X), rs.standard_normal((8, B, 7, 50)), a, b


@pytest.mark.parametrize("condition", [True, False], ids=["pinned", "condition_false"])
def test_device_loop(tiny_net, condition):
    """4. the last 8 steps (two of them guided) of denoise_guided, free-running from a given state at step 8, on the ensemble in which no
    row normalises: every unweighted row bit-identical to the run with weight 0, the weighted rows not; with the end columns pinned the
    stepwise API gives the same bits.  condition=False: the run completes, finite, and its weighted rows differ from the weight-0 run's
    (no claim on where they end)"""
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion, WarmStart, guided_step
    from edmp_amd.guide import IntersectionVolumeGuide

    X8, z, s, gl = loop_inputs()
    assert sum(guided_step(t) for t in range(8, 0, -1)) == 2
    scene = scenes.random_scene(7, 8)
    dif = Diffusion(T, DEV)
    target = I.pose_of(gl, "hand")

    def run(cfgs, **kw):
        guide = IntersectionVolumeGuide(scene, DEV, cfgs, B, goal_tool="hand", **kw)
        X = dif.denoise_guided(tiny_net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=s, goal=gl, noise=z, condition=condition,
                               warm_start=WarmStart(X8, 8, renoise=False))
        return X, guide

    cfgs, cfgs0 = I.mixed_cfgs(48, grad_norm=False), I.mixed_cfgs(48, with_term=False, grad_norm=False)
    assert not cfgs["grad_norm"].any()
    Xg, guide = run(cfgs, goal_target=target)
    X0, _ = run(cfgs0, goal_target=target)
    rows = list(I.GOAL_ROWS)
    others = [r for r in range(B) if r not in rows]
    assert np.isfinite(Xg).all()
    assert np.array_equal(Xg[others], X0[others])
    assert all(not np.array_equal(Xg[r], X0[r]) for r in rows)
    Xd, _ = run(cfgs)  # the derived target is the same pose
    assert np.array_equal(Xd, Xg)
    rep, rep0 = guide.sdf_goal_rows(Xg[:, :, 1:-1]), guide.sdf_goal_rows(X0[:, :, 1:-1])
    record(test="device_loop", condition=condition, weighted_rows_min_distance=rep["min_distance"][rows].tolist(), weight0_min_distance=rep0["min_distance"][rows].tolist())
    if condition:
        X = X8.copy()
        for k, t in enumerate(range(8, 0, -1)):
            X = dif.denoise_step(tiny_net, guide, X, z[k], t, s, gl, cfgs["guidance_schedule"])["x_out"]
        assert np.array_equal(X, Xg)


SCENE_GUIDES = (([1, 101, 10, 101], 1), ([101, 13], 2), ([5, 101], 2))  # B = 4 rows each; scene 1 mixes goal rows with rows that normalise


@pytest.mark.parametrize("derived", [False, True], ids=["explicit", "derived"])
def test_scene_batch_equals_serial_runs(tiny_net, derived):
    """5. three scenes with different obstacle counts, goals and targets, guide 103 at different places: 8 steps (4 guided) of the batch
    equal each scene's serial run bit for bit - raw gradient, sum g^2 and the normalising neighbours all enter the state - and so does
    the report"""
    S, Bs = SI.S, 4
    targets = [None if derived else I.random_pose(40 + s) for s in range(S)]
    rs = np.random.RandomState(SI.NOISE_SEED)
    noises = [rs.standard_normal((T + 1, Bs, 7, SI.N)) for _ in range(S)]
    run = suite.scene_batch_run(TERM, tiny_net, SCENE_GUIDES, noises, 8, each=lambda s: dict(goal_tool=I.CUSTOM_TOOL, goal_target=targets[s]))
    batch, guides, starts, goals, got = run.batch, run.guides, run.starts, run.goals, run.got
    assert batch.batch_size == Bs
    rep = batch.sdf_goal_rows(got)
    fin = batch.sdf_goal_rows(got, final=True)
    for s in range(S):
        if derived:  # the scene's own guide reads the pose of the goal of its last call: hand scene s's pair over again
            guides[s].row_swept_volumes(starts[s], goals[s], got[s])
        one, last = guides[s].sdf_goal_rows(got[s][:, :, 1:-1]), guides[s].sdf_goal_rows(got[s][:, :, 1:])
        for k in ("cost", "distance", "angle", "min_distance"):
            assert rep[k].shape == (S, Bs) and np.array_equal(rep[k][s], one[k]) and np.array_equal(fin[k][s], last[k]), (s, k)
        assert len({float(v) for v in fin["distance"][s]}) == 1  # the pinned goal column: one pose for every row of the scene
    if derived:  # the plan ends at the goal configuration, whose pose is the target
        assert fin["distance"].max() <= 1e-6 and fin["angle"].max() <= 1e-5


def test_scene_batch_refusals():
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch

    parts = SI.scene_parts()[:2]
    cfgs = SI.cfgs_for([103, 13], 2)
    mk = lambda s, **kw: IntersectionVolumeGuide(parts[s]["obstacle_config"], DEV, cfgs, 4, obstacle_kinds=parts[s]["kinds"], bind=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="scene 1.*goal_target"):
        SceneBatch([mk(0, goal_target=I.random_pose(1)), mk(1)])
    with pytest.raises(ValueError, match="scene 1.*goal_target"):
        SceneBatch([mk(0), mk(1, goal_target=I.random_pose(1))])
    with pytest.raises(ValueError, match="scene 1.*goal_tool"):
        SceneBatch([mk(0, goal_tool="flange"), mk(1, goal_tool="hand")])
    assert SceneBatch([mk(0, goal_tool="flange"), mk(1, goal_tool="flange")]).has_term("goal")


# ---- 6. state rules ----------------------------------------------------------------------------------------------------------------------
def test_state_rules_and_refusals():
    from edmp_amd import _capi

    case = I.check_case("L2_flange")
    cfgs, L = case["cfgs"], case["L"]
    w, r, k = (np.ascontiguousarray(a) for a in I.goal_arrays(cfgs))
    k = np.ascontiguousarray(k.astype(np.int32))
    tool = np.ascontiguousarray(I.CUSTOM_TOOL.reshape(12))
    tgt = np.ascontiguousarray(case["target"].reshape(12))
    no_sdf = {key: v for key, v in I.mixed_cfgs(L, with_term=False).items() if not key.startswith("sdf_") and key != "smoothness"}
    plain = build_guide(case, cfgs=no_sdf)
    plain._bind()
    lib, h = plain.ctx.lib, plain.ctx.h

    def call(w_=w, r_=r, k_=k, tool_=tool, tgt_=tgt, n=B):
        return suite.setter_call(TERM, lib, h, _capi.as_pd(np.ascontiguousarray(w_)), _capi.as_pd(np.ascontiguousarray(r_)), _capi.as_pi32(np.ascontiguousarray(k_)),
                                 _capi.as_pd(np.ascontiguousarray(tool_)), None if tgt_ is None else _capi.as_pd(np.ascontiguousarray(tgt_)), n)

    rc, msg = call()  # before the sphere table
    assert rc == -3 and msg.startswith("edmp_sdf_set_goal") and "edmp_sdf_set" in msg, (rc, msg)
    guide = build_guide(case, goal_target=case["target"])
    guide._bind()
    args = (case["joints"], case["start"], case["goal"], I.T_CHECK)
    state = lambda: suite.bound_state(guide, case, guide.sdf_goal_rows(case["joints"]))  # noqa: E731
    before = state()
    w_bad = w.copy()
    w_bad[3] = 1.0  # an iv row
    k_bad = k.copy()
    k_bad[2] = 0
    skew = tool.copy()
    skew[0] += 1e-4
    for what, kw, needle in (("wrong n", dict(n=B - 1), "rows"), ("weight on a non-SDF row", dict(w_=w_bad), "row 3"), ("NaN weight", dict(w_=np.full(B, np.nan)), "weight"),
                             ("negative rotation", dict(r_=-r - 1.0), "rotation"), ("window 0", dict(k_=k_bad), "row 2"), ("tool not orthonormal", dict(tool_=skew), "tool"),
                             ("target not orthonormal", dict(tgt_=2 * tgt), "target")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("edmp_sdf_set_goal") and needle in msg, (what, rc, msg)
    suite.assert_state_is(state(), before)
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_goal_rows_dev"):
        guide.sdf_goal_rows(case["joints"][:3], I.T_CHECK)  # t >= 1: the bound rows
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_goal_rows_dev"):
        guide.sdf_goal_rows(np.zeros((2, 7, 63)), 0)
    # derived targets: the report refuses until a start / goal pair has been handed over
    rc, msg = call(tgt_=None)
    assert rc == 0, msg
    out = plain.ctx.empty((4, B), torch.float64)
    ji = plain.ctx.to_dev(case["joints"], torch.float64)
    rows_dev = lambda: lib.edmp_sdf_goal_rows_dev(h, C.c_void_p(ji.data_ptr()), B, L, 0, L, 0, *(C.c_void_p(out[i].data_ptr()) for i in range(4)))  # noqa: E731
    assert rows_dev() == -3 and b"start / goal" in lib.edmp_last_error()
    guide.get_gradient(*args)
    assert rows_dev() == 0, lib.edmp_last_error()
    plain.ctx.sync()
    # a new sphere table drops the term: the gradient is that of the ensemble without it, and the report asks for edmp_sdf_set_goal again
    suite.a_later_table_drops_the_term(TERM, guide, case, before[1])
    assert rows_dev() == -3 and b"edmp_sdf_set_goal" in lib.edmp_last_error()
    # in a batch the message names the scene and the row inside it
    suite.bind_a_batch_of_two(case)
    rc, msg = call(w_=np.concatenate([w, w_bad]), r_=np.concatenate([r, r]), k_=np.concatenate([k, k]), tgt_=None, n=2 * B)
    assert rc == -1 and "scene 1, row 3" in msg, (rc, msg)


def test_a_segmented_run_goes_on(tiny_net):
    """edmp_sdf_goal_rows_dev between two segments of a segmented run: the run's result is bit-identical to the uninterrupted one, with an
    explicit target and with a derived one"""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = I.mixed_cfgs(48)
    X8, _, s, gl = loop_inputs()
    rs = np.random.RandomState(11)
    for target in (I.pose_of(gl, "flange"), None):
        g = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, B, goal_tool="flange", goal_target=target)
        mid = suite.segmented_run_goes_on(tiny_net, g, cfgs, s, gl, rs, lambda: g.sdf_goal_rows(X8[:, :, 1:-1]))
        assert np.isfinite(mid["cost"]).all() and mid["cost"][list(I.GOAL_ROWS)].all()


def test_driver_report_of_the_chosen_plan(tmp_path):
    """infer_serial with guide 103 in the run config: a problem set that carries target poses hands them over (in the frame --ik-tool
    names) and --ensemble-report adds the chosen plan's position_error [cm] and orientation_error [deg] - evaluation.tool_pose_errors of
    the final column under the report's gates -, scene by scene and for a group in one launch; without targets the pose of the picked
    goal is the target and the pinned final column sits on it"""
    import yaml

    import infer_serial
    from edmp_amd import evaluation as EV
    from edmp_amd import franka, scenes
    from edmp_amd.guide import goal_pose

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lo, hi = franka.joint_limits()
    rs = np.random.RandomState(9)
    problems = []
    for k in range(2):
        oc = scenes.random_scene(20 + k, 6)
        to_wxyz = lambda o: [float(o[6]), float(o[3]), float(o[4]), float(o[5])]  # noqa: E731
        xyz, quat = I.random_pose(60 + k)
        problems.append({"cuboids": [{"center": o[:3].tolist(), "quaternion_wxyz": to_wxyz(o), "dims": o[7:10].tolist()} for o in oc[:4]],
                         "cylinders": [{"center": o[:3].tolist(), "quaternion_wxyz": to_wxyz(o), "radius": float(o[7]), "height": float(o[9])} for o in oc[4:]],
                         "start": rs.uniform(lo, hi).tolist(), "target": {"xyz": xyz.tolist(), "quaternion_wxyz": quat.tolist()},
                         "goals": rs.uniform(lo, hi, (5, 7)).tolist()})
    pj = tmp_path / "problems.json"
    json.dump({"format": "edmp_amd problem set v1", "scene_types": {"tabletop": problems}}, open(pj, "w"))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "cfg_c1_plumbing.yaml")))
    cfg["guide"]["guides"], cfg["guide"]["batch_size_per_guide"] = [1, 103], 2
    os.makedirs(tmp_path / "cfgs")
    c_syn = tmp_path / "cfgs" / "cfg_synthetic.yaml"
    yaml.safe_dump(cfg, open(c_syn, "w"))
    cfg["dataset"]["scene_types"] = ["tabletop"]
    c_set = tmp_path / "cfgs" / "cfg_problem_set.yaml"
    yaml.safe_dump(cfg, open(c_set, "w"))
    ds = scenes.ProblemSetDataset(str(pj))
    for kw in (dict(), dict(scenes_per_launch=2)):
        np.random.seed(5)
        res = infer_serial.run(str(c_set), dataset=ds, verbose=False, ensemble_report=True, ik_tool="hand", **kw)
        assert len(res) == 2
        for k, r in enumerate(res):
            target = (np.asarray(problems[k]["target"]["xyz"]), np.asarray(problems[k]["target"]["quaternion_wxyz"]))
            host = EV.tool_pose_errors(r["trajectory"][:, -1], target, "hand")
            cols = r["trajectory"][None, :, 1:]
            one = (np.ones(1), np.ones(1), np.full(1, cols.shape[2]))
            tg = goal_pose(target)
            ev = I.evaluate_goal(cols, tg, "hand", *one, want_grad=False)
            y = I.report_yardstick(cols, tg, "hand", *one, ev)
            assert ev["distance"][0] == host["distance"] and ev["angle"][0] == host["angle"]
            derr, aerr = abs(r["position_error"] / 100 - host["distance"]), abs(math.radians(r["orientation_error"]) - host["angle"])
            record(test="driver_report", scenes_per_launch=kw.get("scenes_per_launch", 1), scene=k, position_error_cm=r["position_error"],
                   orientation_error_deg=r["orientation_error"], distance_abs_err=derr, angle_abs_err=aerr,
                   gate_abs=[I.abs_gate(y["distance_abs"], ev["coord_max"]), I.abs_gate(y["angle_abs"], math.pi)])
            assert derr <= I.abs_gate(y["distance_abs"], ev["coord_max"]) and aerr <= I.abs_gate(y["angle_abs"], math.pi) + 1e-12
    np.random.seed(5)
    res = infer_serial.run(str(c_syn), verbose=False, ensemble_report=True, max_scenes=1)
    assert res[0]["position_error"] <= 100 * 1e-6 and res[0]["orientation_error"] <= math.degrees(1e-5)
    np.random.seed(5)
    plain = infer_serial.run(os.path.join(root, "configs", "cfg_c1_plumbing.yaml"), verbose=False, ensemble_report=True, max_scenes=1)
    assert "position_error" not in plain[0]
