"""The swept-clearance term of the sphere signed-distance guide (sdf_sweep_kernel, edmp_sdf_set_sweep, edmp_sdf_sweep_rows_dev,
edmp_scenes_sdf_sweep_rows_dev) on the GPU against its float64 checker (tests/sdf_sweep_inputs.py).

Gate: sdf_reference.gate - max(4 x the deviation of the checker's own formula in CPU float32 from float64, 4 f32 ulps), relative to
the largest element (for the minimum clearance: absolute, with the floor of a few f32 ulps of the largest coordinate that enters it,
as sdf_reference.clearance_gate).  Every comparison prints its error, yardstick and gate; with EDMP_SDF_SWEEP_PARITY_OUT=<file> the
records are written there as JSON (profiles/sdf_sweep_parity.json comes from such a run).  Waypoints and interpolants sit >= 1e-5 m
from every kink, so no element is excluded from any comparison."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import scene_sdf_inputs as SI
from tests import sdf_reference as R
from tests import sdf_sweep_inputs as I
from tests import sdf_term_suite as suite
from tests.sdf_gpu import DEV, build_guide, recorder, run_cfgs, tiny_net  # noqa: F401  (tiny_net: this module's fixture)

pytestmark = pytest.mark.gpu
T, B = I.T, I.B
record, _write_records = recorder("sdf sweep parity", "EDMP_SDF_SWEEP_PARITY_OUT",
                                  "max(4 x CPU-float32 deviation from float64, 4 f32 ulps), relative to the largest element; clearance: absolute, "
                                  "floor 4 f32 ulps of the largest coordinate")
TERM = suite.Term("sweep", I, guide=104, rows=I.SWEEP_ROWS, gradient_yardstick=lambda case: I.yardstick(case, I.T_CHECK)["grad"],
                  report=lambda g, X, start, goal, t, substeps=None: g.sdf_sweep_rows(X, start, goal, t, substeps=substeps),
                  gradient_record=lambda case: dict(substeps=list(case["K"]), active_share=case["marginst"]["active"]),
                  report_steps=((0, dict(substeps=None)), (R.T_CHECK, dict(substeps=None)), (0, dict(substeps=3))))


@pytest.mark.parametrize("t", [0, I.T_CHECK])
@pytest.mark.parametrize("name", list(I.CASES))
def test_cost_and_clearance_of_every_row(name, t):
    """1. sdf_sweep_rows against the checker at t = 0 (margin 0) and at a step of the non-constant margin schedule, every row with its
    own weight and substeps; at t = 0 also substeps= on rows that are not the bound ones (weight 1)"""
    case = I.check_case(name)
    guide = build_guide(case)
    assert guide.has_term("sweep")
    ev = case["sweep0"] if t == 0 else case["sweept"]
    out = guide.sdf_sweep_rows(case["joints"], case["start"], case["goal"], t)
    y = I.yardstick(case, t)
    scale = float(np.abs(ev["cost"]).max())
    cost_err = float(np.abs(out["cost"] - ev["cost"]).max())
    cgate = R.clearance_gate(y["clearance_abs"], ev["coord_max"])
    clr_err = float(np.abs(out["clearance"] - ev["clearance"]).max())
    record(test="cost_clearance", case=name, t=t, cost_abs_err=cost_err, cost_scale=scale, cost_yardstick=y["cost"], cost_gate=R.gate(y["cost"]),
           clearance_abs_err=clr_err, clearance_yardstick_abs=y["clearance_abs"], clearance_gate_abs=cgate, min_clearance=float(ev["clearance"].min()))
    assert out["cost"].shape == (B,) and out["cost"].dtype == np.float64
    assert cost_err <= R.gate(y["cost"]) * scale, (cost_err, scale, y["cost"])
    assert clr_err <= cgate, (clr_err, cgate)
    assert not out["cost"][[r for r in range(B) if r not in I.SWEEP_ROWS]].any()  # weight 0
    if t == 0:
        n, K = I.UNBOUND_ROWS, case["K"][0]
        bare = case["every0"]
        sub = guide.sdf_sweep_rows(case["joints"][:n], case["start"], case["goal"], 0, substeps=K)
        b32 = I.evaluate_sweep(case["joints"][:n], *case["args"][1:], np.zeros(n), np.ones(n), K, dtype=torch.float32, want_grad=False)
        bscale = float(np.abs(bare["cost"]).max())
        yb = float(np.abs(b32["cost"] - bare["cost"]).max()) / max(bscale, 1e-300)
        yc = float(np.abs(b32["clearance"] - bare["clearance"]).max())
        berr, cerr = float(np.abs(sub["cost"] - bare["cost"]).max()), float(np.abs(sub["clearance"] - bare["clearance"]).max())
        record(test="cost_unbound_rows", case=name, substeps=K, cost_abs_err=berr, cost_scale=bscale, cost_yardstick=yb, cost_gate=R.gate(yb),
               clearance_abs_err=cerr, clearance_gate_abs=R.clearance_gate(yc, bare["coord_max"]))
        assert berr <= R.gate(yb) * max(bscale, 1e-300), (berr, bscale, yb)
        assert cerr <= R.clearance_gate(yc, bare["coord_max"]), cerr


def test_the_plate():
    """2. positive clearance at every waypoint, a link swept through a thin plate between two of them: sdf_rows reports the former,
    sdf_sweep_rows the latter; under a margin below the waypoint clearance the guide without the term has a zero gradient on the row,
    with the term a non-zero one that matches the checker"""
    p = I.plate_case()
    args = (p["joints2"], p["start"], p["goal"])  # (row 1 rests inside the plate and keeps the batch's ||g|| away from 0)
    plain, swept = build_guide(p, cfgs=I.plate_cfgs(False)), build_guide(p, cfgs=I.plate_cfgs(True))
    way = plain.sdf_rows(*args, 0)["clearance"][0]
    sw = swept.sdf_sweep_rows(*args, 0)["clearance"][0]
    also = plain.sdf_sweep_rows(p["joints"], p["start"], p["goal"], 0, substeps=I.PLATE_K)["clearance"][0]  # a guide without the term, the check's substeps handed in
    e32 = I.evaluate_sweep(*p["args"], np.zeros(1), np.ones(1), I.PLATE_K, dtype=torch.float32, want_grad=False)
    cg = R.clearance_gate(abs(e32["clearance"][0] - p["sweep0"]["clearance"][0]), p["sweep0"]["coord_max"])
    assert way > 0.07 and sw < -0.04 and also == sw
    assert abs(sw - p["sweep0"]["clearance"][0]) <= cg and abs(way - p["way0"]["clearance"][0]) <= R.GATE_FLOOR * p["way0"]["coord_max"] + cg
    G0 = plain.get_gradient(*args, I.T_CHECK)
    G = swept.get_gradient(*args, I.T_CHECK)
    assert np.isfinite(G0).all() and not G0[0].any() and G0[1].any() and np.array_equal(G[1], G0[1])
    G = G[:1]
    ref = p["sweep"]["grad"]
    g32 = I.evaluate_sweep(*p["args"], np.full(1, I.PLATE_MARGIN), np.ones(1), I.PLATE_K, dtype=torch.float32)["grad"]
    scale = float(np.abs(ref).max())
    y = float(np.abs(g32 - ref).max()) / scale
    err = float(np.abs(G - ref).max()) / scale
    record(test="plate", waypoint_clearance=float(way), swept_clearance=float(sw), grad_rel_err=err, yardstick=y, gate=R.gate(y))
    assert scale > 0 and G.any() and err <= R.gate(y), (err, y)


@pytest.mark.parametrize("name", list(I.CASES))
def test_gradient_of_a_mixed_ensemble(name):
    """3. get_gradient on SDF + sweep (two rows, their own K), plain SDF, iv and sv rows, with and without grad_norm: the weighted rows
    against the checker (the normalising one un-normalised by the device's own sum g^2), bit-identical on a second call, every other row
    that does not normalise BIT-identical to the same ensemble built without the term"""
    suite.gradient_of_a_mixed_ensemble(TERM, record, name)


@pytest.mark.parametrize("name", ["L1_o1_custom_K2", "L48_o64_default_K42", "L62_o7c2_default_K8"])
def test_rowsq_is_the_sum_of_the_final_squares(name):
    """4. the sum g^2 the norm mixing reads, on an ensemble in which no row normalises (the returned gradient is the raw one): math.fsum
    of the returned squares to 8 x 2^-24 - seven f32 fmaf per lane, then f64 sums"""
    suite.rowsq_is_the_sum_of_the_final_squares(TERM, record, name)


def test_ends():
    """5. a gradient placed by the start -> q_1 segment alone: only waypoint 1 moves, by the second-set weights (the first-set part
    belongs to the pinned start and is dropped); the rows beside it keep the bits they have without the term"""
    from edmp_amd import guide_cfg as GC

    e = I.ends_case()
    args = (e["joints"], e["start"], e["goal"], 0)
    G = build_guide(e, cfgs=I.ends_cfgs()).get_gradient(*args)
    ref = e["sweep"]["grad"]
    g32 = I.evaluate_sweep(*e["args"], np.zeros(1), np.ones(1), 4, dtype=torch.float32)["grad"]
    scale = float(np.abs(ref).max())
    y = float(np.abs(g32 - ref).max()) / scale
    err = float(np.abs(G - ref).max()) / scale
    record(test="ends", grad_rel_err=err, yardstick=y, gate=R.gate(y))
    assert G[0, :, 0].any() and not G[0, :, 1:].any() and err <= R.gate(y), (G, err, y)
    # the row between two others: what lies before and behind [r][7][L] is theirs and keeps its bits
    # (at a step t >= 1, where row 0's margin of 0.5 m makes its waypoint hinge active: the batch's ||g|| is not 0 without the term either)
    def three(sweep):
        d = [R.guide_dict("sdf", False, 0.0, 410), R.guide_dict("sdf", False, 0.0, 411), R.guide_dict("sv", False, 0.0, 412)]
        d[0]["hyperparameters"]["sdf"].update(margin=[0.5, 0.5])
        d[1]["hyperparameters"]["sdf"].update(margin=[0.0, 0.0], **(dict(sweep_weight=1.0, sweep_substeps=4) if sweep else {}))
        return GC.build_guide_cfgs(d, 1, T)

    J = np.repeat(e["joints"], 3, axis=0)
    G3 = build_guide(e, cfgs=three(True)).get_gradient(J, e["start"], e["goal"], I.T_CHECK)
    G30 = build_guide(e, cfgs=three(False)).get_gradient(J, e["start"], e["goal"], I.T_CHECK)
    assert np.isfinite(G30).all() and G30[0].any()
    assert np.array_equal(G3[[0, 2]], G30[[0, 2]]) and np.array_equal(G3[1], G[0]) and not G30[1].any()


# ---- runs --------------------------------------------------------------------------------------------------------------------------
def test_scene_batch_equals_serial_runs(tiny_net):
    """6. three scenes with guide 104 at different places (beside guide 13, whose rows normalise by the scene's ||g||): 24 guided steps of
    the batch equal each scene's serial run bit for bit, differ from the run without the term, and so does the report"""
    suite.scene_batch_equals_serial_runs(TERM, tiny_net)


def test_device_loop_equals_the_stepwise_api(tiny_net):
    """7. six steps (three of them guided) of the device loop against edmp_step_a_dev / edmp_step_b_dev, guide 104 beside guides 1 and 13"""
    suite.device_loop_equals_the_stepwise_api(TERM, tiny_net)


def test_full_run_with_guide_104(tiny_net):
    """8. all 255 steps with guide 104 between guides 1 and 13: finite, bit-identical when repeated, not the run of guide 101 on guide
    104's rows and the same on guide 1's"""
    suite.full_run(TERM, tiny_net)


def test_a_segmented_run_goes_on(tiny_net):
    """8. a report call - with another start / goal pair than the run's - between two segments of a segmented run: the run's result is
    bit-identical to the uninterrupted one"""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = run_cfgs(104)
    Bn = cfgs["total_batch_size"]
    s, gl = np.asarray(scenes.DEFAULT_START, dtype=np.float64), np.asarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    rs = np.random.RandomState(11)
    g = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, Bn)

    def between():  # (called once, after the noise of both segments has been drawn from rs)
        X = rs.uniform(-1, 1, (Bn, 7, 48))
        return g.sdf_sweep_rows(X, gl, s, 0), g.sdf_sweep_rows(X[:3], gl, s, 0, substeps=5)

    mid = suite.segmented_run_goes_on(tiny_net, g, cfgs, s, gl, rs, between)
    assert np.isfinite(mid[0]["clearance"]).all() and np.isfinite(mid[1]["clearance"]).all()


def test_refusals():
    """9. every misuse is an error return whose message names the entry point, and the bound state is what it was"""
    from edmp_amd import _capi
    from edmp_amd.runtime import ptr

    case = I.check_case("L2_o7c2_default_K4")
    cfgs = case["cfgs"]
    args = (case["joints"], case["start"], case["goal"])
    no_keys = {k: v for k, v in I.mixed_cfgs(case, with_term=False).items() if k not in SI.SDF_KEYS}
    plain = build_guide(case, cfgs=no_keys)
    plain._bind()
    lib, h = plain.ctx.lib, plain.ctx.h
    w, k = np.ascontiguousarray(cfgs["sdf_sweep_weight"]), np.ascontiguousarray(cfgs["sdf_sweep_substeps"].astype(np.int32))

    def call(w_=w, k_=k, n=B):
        return suite.setter_call(TERM, lib, h, _capi.as_pd(np.ascontiguousarray(w_)), _capi.as_pi32(np.ascontiguousarray(k_)), n)

    rc, msg = call()  # before edmp_sdf_set
    assert rc == -3 and msg.startswith("edmp_sdf_set_sweep") and "edmp_sdf_set" in msg, (rc, msg)
    guide = build_guide(case)
    guide._bind()
    state = lambda: suite.bound_state(guide, case, guide.sdf_sweep_rows(*args, I.T_CHECK))  # noqa: E731
    before = state()
    w_bad = w.copy()
    w_bad[3] = 1.0  # an iv row
    k1, k65 = k.copy(), k.copy()
    k1[0], k65[1] = 1, 65
    for what, kw, needle in (("wrong n", dict(n=B - 1), "rows"), ("weight on a non-SDF row", dict(w_=w_bad), "row 3"), ("K = 1", dict(k_=k1), "row 0"),
                             ("K = 65", dict(k_=k65), "row 1"), ("NaN weight", dict(w_=np.full(B, np.nan)), "weight"), ("negative weight", dict(w_=-w - 1.0), "weight")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("edmp_sdf_set_sweep") and needle in msg, (what, rc, msg)
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_sweep_rows_dev"):
        guide.sdf_sweep_rows(*args, I.T_CHECK, substeps=4)  # substeps > 0 at t >= 1
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_sweep_rows_dev"):
        guide.sdf_sweep_rows(case["joints"][:3], case["start"], case["goal"], 0)  # the rows' own substeps on rows that are not the bound ones
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_sweep_rows_dev"):
        guide.sdf_sweep_rows(*args, 0, substeps=65)
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_sweep_rows_dev"):
        guide.sdf_sweep_rows(np.zeros((2, 7, 63)), case["start"], case["goal"], 0, substeps=4)
    suite.assert_state_is(state(), before)
    # a later edmp_sdf_set drops the term: the gradient is that of the ensemble without it, and the report asks for the row arrays again
    suite.a_later_table_drops_the_term(TERM, guide, case, before[1])
    out = guide.ctx.empty((2, B), torch.float64)
    Xd = guide.ctx.to_dev(case["joints"], torch.float64)
    s7, g7 = _capi.as_pd(np.ascontiguousarray(case["start"])), _capi.as_pd(np.ascontiguousarray(case["goal"]))
    rc = lib.edmp_sdf_sweep_rows_dev(h, ptr(Xd), B, case["L"], 0, s7, g7, 0, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()))
    assert rc == -3 and (lib.edmp_last_error() or b"").decode().startswith("edmp_sdf_sweep_rows_dev") and b"edmp_sdf_set_sweep" in lib.edmp_last_error()
    # in a batch the message names the scene and the row inside it
    suite.bind_a_batch_of_two(case)
    rc, msg = call(w_=np.concatenate([w, w_bad]), k_=np.concatenate([k, k]), n=2 * B)
    assert rc == -1 and msg.startswith("edmp_sdf_set_sweep") and "scene 1, row 3" in msg, (rc, msg)
    rc, msg = call(w_=np.concatenate([w, w]), k_=np.concatenate([k, k65]), n=2 * B)
    assert rc == -1 and "scene 1, row 1" in msg, (rc, msg)


def test_driver_report_of_the_chosen_plan(tmp_path):
    """infer_serial --ensemble-report on a config that lists guide 104: the chosen plan's min_swept_clearance next to min_clearance, the
    same from the serial loop and from the scene-group path (one batch call), and what the guide itself reports for that row"""
    import yaml

    import infer_serial
    from edmp_amd import scenes

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "cfg_c1_plumbing.yaml")))
    cfg["guide"]["guides"] = [1, 104]
    path = str(tmp_path / "cfg_sweep.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    out = []
    for k in (1, 2):
        np.random.seed(31)
        ds = scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=2, n_obstacles=6, n_cylinders=1)
        out.append(infer_serial.run(path, dataset=ds, verbose=False, scenes_per_launch=k, ensemble_report=True))
    assert len(out[0]) == len(out[1]) == 2
    for a, b in zip(*out):
        assert np.array_equal(a["trajectory"], b["trajectory"]) and a["best_row"] == b["best_row"]
        assert np.isfinite(a["min_swept_clearance"]) and a["min_swept_clearance"] == b["min_swept_clearance"] and a["min_clearance"] == b["min_clearance"]
