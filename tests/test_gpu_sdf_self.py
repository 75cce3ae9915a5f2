"""The self-clearance term of the sphere signed-distance guide (sdf_self_kernel, edmp_sdf_set_self, edmp_sdf_self_rows_dev) on the GPU
against its float64 autograd checker (tests/sdf_self_inputs.py).

Gate: sdf_reference.gate - max(4 x the deviation of the checker's own formula in CPU float32 from float64, 4 f32 ulps), relative to
the largest element (for the minimum clearance: to the largest sphere-centre coordinate, see the helper).  Every comparison prints its
error, yardstick and gate; with EDMP_SDF_SELF_PARITY_OUT=<file> the records are written there as JSON (profiles/sdf_self_parity.json
comes from such a run).  The inputs sit >= 1e-5 m from every kink, so no element is excluded from any comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scene_sdf_inputs as SI
from tests import sdf_reference as R
from tests import sdf_self_inputs as I
from tests import sdf_term_suite as suite
from tests.sdf_gpu import build_guide, recorder, tiny_net  # noqa: F401  (tiny_net: this module's fixture)

pytestmark = pytest.mark.gpu
T, B = I.T, I.B
record, _write_records = recorder("sdf self parity", "EDMP_SDF_SELF_PARITY_OUT",
                                  "max(4 x CPU-float32 deviation from float64, 4 f32 ulps), relative to the largest element")
TERM = suite.Term("self", I, guide=102, rows=I.SELF_ROWS, report=lambda g, X, start, goal, t: g.sdf_self_rows(X, t),
                  gradient_yardstick=lambda case: I.yardstick(case, I.T_CHECK)["grad"],
                  gradient_record=lambda case: dict(active_share=case["marginst"]["active"]))


@pytest.mark.parametrize("t", [0, I.T_CHECK])
@pytest.mark.parametrize("name", list(I.CASES))
def test_cost_and_clearance_of_every_row(name, t):
    """1. sdf_self_rows against the checker at t = 0 (margin 0) and at a step of the non-constant margin schedule, every row"""
    case = I.check_case(name)
    guide = build_guide(case)
    ev = case["self0"] if t == 0 else case["selft"]
    out = guide.sdf_self_rows(case["joints"], t)
    y = I.yardstick(case, t)
    scale = float(np.abs(ev["cost"]).max())
    cost_err = float(np.abs(out["cost"] - ev["cost"]).max())
    cgate = R.clearance_gate(y["clearance_abs"], ev["coord_max"])
    clr_err = float(np.abs(out["clearance"] - ev["clearance"]).max())
    record(test="cost_clearance", case=name, t=t, cost_abs_err=cost_err, cost_scale=scale, cost_yardstick=y["cost"], cost_gate=R.gate(y["cost"]),
           clearance_abs_err=clr_err, clearance_yardstick_abs=y["clearance_abs"], clearance_gate_abs=cgate)
    assert out["cost"].shape == (B,) and out["cost"].dtype == np.float64
    assert cost_err <= R.gate(y["cost"]) * scale, (cost_err, scale, y["cost"])
    assert clr_err <= cgate, (clr_err, cgate)
    assert not out["cost"][[r for r in range(B) if r not in I.SELF_ROWS]].any()  # weight 0
    if t == 0:  # any n at t = 0: rows that are not the bound ones carry weight 1
        sub = guide.sdf_self_rows(case["joints"][:3], 0)
        bare = I.evaluate_self(case["joints"][:3], case["spheres"], case["mask"], np.zeros(3), np.ones(3), want_grad=False)
        b32 = I.evaluate_self(case["joints"][:3], case["spheres"], case["mask"], np.zeros(3), np.ones(3), dtype=torch.float32, want_grad=False)
        bscale = float(np.abs(bare["cost"]).max())  # (this sum's own yardstick: the same formula in CPU float32)
        yb = float(np.abs(b32["cost"] - bare["cost"]).max()) / max(bscale, 1e-300)
        berr = float(np.abs(sub["cost"] - bare["cost"]).max())
        record(test="cost_unbound_rows", case=name, cost_abs_err=berr, cost_scale=bscale, cost_yardstick=yb, cost_gate=R.gate(yb))
        assert berr <= R.gate(yb) * bscale, (berr, bscale, yb)
        assert np.array_equal(sub["clearance"], out["clearance"][:3])


def test_empty_mask_and_report_on_a_guide_without_the_term():
    """an all-zero mask selects no pair: cost 0 and clearance +inf; a guide without any weight reports with the default mask"""
    case = I.check_case("L2_default")
    out = build_guide(case, self_pairs=np.zeros((9, 9))).sdf_self_rows(case["joints"], I.T_CHECK)
    assert not out["cost"].any() and np.isposinf(out["clearance"]).all()
    plain = build_guide(case, cfgs=I.mixed_cfgs(case, with_term=False))
    assert not plain.has_term("self")
    rep = plain.sdf_self_rows(case["joints"], 0)
    assert np.array_equal(rep["clearance"], build_guide(case).sdf_self_rows(case["joints"], 0)["clearance"]) and not rep["cost"].any()


@pytest.mark.parametrize("name", list(I.CASES))
def test_gradient_of_a_mixed_ensemble(name):
    """2. get_gradient on SDF + self, plain SDF, iv and sv rows, with and without grad_norm: the weighted rows against the checker (the
    normalised one un-normalised by the device's own sum g^2), every other row that does not normalise BIT-identical to the same ensemble
    built without the self table"""
    suite.gradient_of_a_mixed_ensemble(TERM, record, name)


@pytest.mark.parametrize("name", ["L2_default", "L48_custom", "L62_default"])
def test_rowsq_is_the_sum_of_the_final_squares(name):
    """the sum g^2 the norm mixing reads, on an ensemble in which no row normalises (the returned gradient is the raw one): math.fsum of
    the returned squares to 8 x 2^-24 - seven f32 fmaf per lane, then f64 sums"""
    suite.rowsq_is_the_sum_of_the_final_squares(TERM, record, name)


@pytest.mark.parametrize("pair", [(0, 4), (1, 8), (3, 6)])
def test_joints_at_or_below_the_lower_link_contribute_nothing(pair):
    """the claim behind the kernel's joint range: for a single masked link pair the checker - which differentiates the whole expression -
    gives a zero gradient for every joint at or below the lower link's frame (and above the upper link's), below the gate"""
    from edmp_amd import franka

    case = I.check_case("L48_default")
    mask = np.zeros((9, 9), dtype=int)
    mask[pair] = 1
    m, w = np.full(B, 0.5), np.ones(B)
    ev = I.evaluate_self(case["joints"], case["spheres"], mask, m, w)
    e32 = I.evaluate_self(case["joints"], case["spheres"], mask, m, w, dtype=torch.float32)
    scale = float(np.abs(ev["grad"]).max())
    assert scale > 0
    y = float(np.abs(e32["grad"] - ev["grad"]).max()) / scale
    fa, fb = int(franka.LINK_FRAME[pair[0]]), int(franka.LINK_FRAME[pair[1]])
    idle = [j for j in range(7) if j <= fa or j > fb]
    worst = float(np.abs(ev["grad"][:, idle]).max()) / scale
    record(test="zero_contribution", pair=list(pair), idle_joints=idle, rel=worst, gate=R.gate(y))
    assert worst <= R.gate(y), (worst, y)
    assert all(np.abs(ev["grad"][:, j]).max() > 0 for j in range(fa + 1, fb + 1))
    # and the kernel on the same single pair: its report and gradient see the pair's terms only
    out = build_guide(case, self_pairs=mask).sdf_self_rows(case["joints"], 0)
    bare = I.evaluate_self(case["joints"], case["spheres"], mask, np.zeros(B), case["cfgs"]["sdf_self_weight"], want_grad=False)
    assert float(np.abs(out["clearance"] - bare["clearance"]).max()) <= R.clearance_gate(float(np.abs(e32["clearance"] - ev["clearance"]).max()), ev["coord_max"])


# ---- runs --------------------------------------------------------------------------------------------------------------------------
def test_scene_batch_equals_serial_runs(tiny_net):
    """3. three scenes with guide 102 at different places (beside guide 13, whose rows normalise by the scene's ||g||): 24 guided steps of
    the batch equal each scene's serial run bit for bit - raw gradient, sum g^2 and the normalising neighbours all enter the state - and so
    does the report"""
    suite.scene_batch_equals_serial_runs(TERM, tiny_net)


def test_device_loop_equals_the_stepwise_api(tiny_net):
    """4. six steps (three of them guided) of the device loop against edmp_step_a_dev / edmp_step_b_dev, guide 102 beside a normalising one"""
    suite.device_loop_equals_the_stepwise_api(TERM, tiny_net)


def test_full_run_with_guide_102(tiny_net):
    """5. all 255 steps with guide 102 between guides 1 and 13: finite, bit-identical when repeated, not the run of guide 101, and a
    report that leaves a segmented run running"""
    suite.full_run(TERM, tiny_net)


def test_refusals():
    """6. every misuse is an error return whose message names the entry point, and the bound state is what it was"""
    from edmp_amd import _capi
    from edmp_amd.guide import SceneBatch

    case = I.check_case("L2_default")
    cfgs = case["cfgs"]
    plain = build_guide(case, cfgs={k: v for k, v in I.mixed_cfgs(case, with_term=False).items() if k not in SI.SDF_KEYS})
    plain._bind()
    lib, h = plain.ctx.lib, plain.ctx.h
    mask = np.ascontiguousarray(case["mask"].astype(np.int32).reshape(81))
    w, m = np.ascontiguousarray(cfgs["sdf_self_weight"]), np.ascontiguousarray(cfgs["sdf_self_margin"])

    def call(mask_=mask, w_=w, m_=m, n=B, T_=T):
        return suite.setter_call(TERM, lib, h, _capi.as_pi32(mask_), _capi.as_pd(np.ascontiguousarray(w_)), _capi.as_pd(np.ascontiguousarray(m_)), n, T_)

    rc, msg = call()  # before edmp_sdf_set
    assert rc == -3 and msg.startswith("edmp_sdf_set_self") and "edmp_sdf_set" in msg, (rc, msg)
    guide = build_guide(case)
    guide._bind()
    state = lambda: suite.bound_state(guide, case, guide.sdf_self_rows(case["joints"], I.T_CHECK))  # noqa: E731
    before = state()
    w_bad = w.copy()
    w_bad[3] = 1.0  # an iv row
    bad_mask = mask.copy()
    bad_mask[0 * 9 + 5] = 2
    for what, kw, needle in (("wrong n", dict(n=B - 1), "rows"), ("wrong T", dict(T_=T - 1), "steps"), ("weight on a non-SDF row", dict(w_=w_bad), "row 3"),
                             ("negative margin", dict(m_=-m - 1.0), "self_margin"), ("NaN weight", dict(w_=np.full(B, np.nan)), "weight"),
                             ("mask entry 2", dict(mask_=bad_mask), "pair_mask")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("edmp_sdf_set_self") and needle in msg, (what, rc, msg)
    suite.assert_state_is(state(), before)
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_self_rows_dev"):
        guide.sdf_self_rows(case["joints"][:3], I.T_CHECK)  # t >= 1 reads the rows' schedules
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_self_rows_dev"):
        guide.sdf_self_rows(np.zeros((2, 7, 63)), 0)
    # a later edmp_sdf_set drops the term: the gradient is that of the ensemble without it, and the report asks for the table again
    suite.a_later_table_drops_the_term(TERM, guide, case, before[1])
    out = plain.ctx.empty((2, B), torch.float64)
    rc = lib.edmp_sdf_self_rows_dev(h, None, B, 2, 0, 2, 0, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()))
    assert rc == -3 and b"edmp_sdf_set_self" in lib.edmp_last_error()
    # a batch whose members disagree on the mask is refused before anything is bound
    other = np.array(case["mask"])
    other[0, 3] = False
    a, b = build_guide(case, bind=False), build_guide(case, bind=False, self_pairs=other)
    bound = plain.ctx.bound_guide
    with pytest.raises(ValueError, match="self_pairs"):
        SceneBatch([a, b])
    assert plain.ctx.bound_guide is bound
    # in a batch the message names the scene and the row inside it
    suite.bind_a_batch_of_two(case)
    rc, msg = call(w_=np.concatenate([w, w_bad]), m_=np.concatenate([m, m]), n=2 * B)
    assert rc == -1 and "scene 1, row 3" in msg, (rc, msg)
