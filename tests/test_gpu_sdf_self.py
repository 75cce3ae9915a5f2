"""The self-clearance term of the sphere signed-distance guide (sdf_self_kernel, edmp_sdf_set_self, edmp_sdf_self_rows_dev) on the GPU
against its float64 autograd checker (tests/sdf_self_inputs.py).

Gate: sdf_reference.gate - max(4 x the deviation of the checker's own formula in CPU float32 from float64, 4 f32 ulps), relative to
the largest element (for the minimum clearance: to the largest sphere-centre coordinate, see the helper).  Every comparison prints its
error, yardstick and gate; with EDMP_SDF_SELF_PARITY_OUT=<file> the records are written there as JSON (profiles/sdf_self_parity.json
comes from such a run).  The inputs sit >= 1e-5 m from every kink, so no element is excluded from any comparison."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import scene_sdf_inputs as SI
from tests import sdf_reference as R
from tests import sdf_self_inputs as I
from tests.sdf_gpu import DEV, build_guide, gradient_and_sumsq, recorder
from tests.util import TINY_DIMS, noise_for

pytestmark = pytest.mark.gpu
T, B = I.T, I.B
record, _write_records = recorder("sdf self parity", "EDMP_SDF_SELF_PARITY_OUT",
                                  "max(4 x CPU-float32 deviation from float64, 4 f32 ulps), relative to the largest element")


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
    cgate = max(R.GATE_FACTOR * y["clearance_abs"], R.GATE_FLOOR * ev["coord_max"])
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
    plain = build_guide(case, cfgs=I.mixed_cfgs(False))
    assert not plain.has_self_term
    rep = plain.sdf_self_rows(case["joints"], 0)
    assert np.array_equal(rep["clearance"], build_guide(case).sdf_self_rows(case["joints"], 0)["clearance"]) and not rep["cost"].any()


@pytest.mark.parametrize("name", list(I.CASES))
def test_gradient_of_a_mixed_ensemble(name):
    """2. get_gradient on SDF + self, plain SDF, iv and sv rows, with and without grad_norm: the weighted rows against the checker (the
    normalised one un-normalised by the device's own sum g^2), every other row that does not normalise BIT-identical to the same ensemble
    built without the self table"""
    case = I.check_case(name)
    t, cfgs = I.T_CHECK, case["cfgs"]
    y = I.yardstick(case, t)
    ref = I.total_gradient(case)
    args = (case["joints"], case["start"], case["goal"], t)
    G, sq = gradient_and_sumsq(build_guide(case), *args)
    G_again, sq_again = gradient_and_sumsq(build_guide(case), *args)
    G0, sq0 = gradient_and_sumsq(build_guide(case, cfgs=I.mixed_cfgs(False)), *args)
    assert G.shape == ref.shape and np.isfinite(G).all()
    assert np.array_equal(G, G_again) and sq == sq_again  # one order of every sum
    rows = list(I.SELF_ROWS)
    scale = float(np.abs(ref[rows]).max())
    err = {}
    for r in rows:
        raw = G[r] * float(np.float32(math.sqrt(sq))) if cfgs["grad_norm"][r] else G[r]
        err[r] = float(np.abs(raw - ref[r]).max()) / scale
    record(test="gradient", case=name, t=t, row_rel_err=err, yardstick=y["grad"], gate=R.gate(y["grad"]), active_share=case["marginst"]["active"],
           self_share_of_gradient=float(np.abs(case["selft"]["grad"][rows]).max() / scale))
    for r in rows:
        assert err[r] <= R.gate(y["grad"]), (r, err[r], y["grad"])
        assert not np.array_equal(G[r], G0[r])  # the term does reach the row
    assert sq != sq0
    for r in range(B):
        if r not in rows and not cfgs["grad_norm"][r]:
            assert np.array_equal(G[r], G0[r]), r


@pytest.mark.parametrize("name", ["L2_default", "L48_custom", "L62_default"])
def test_rowsq_is_the_sum_of_the_final_squares(name):
    """the sum g^2 the norm mixing reads, on an ensemble in which no row normalises (the returned gradient is the raw one): math.fsum of
    the returned squares to 8 x 2^-24 - seven f32 fmaf per lane, then f64 sums"""
    case = I.check_case(name)
    cfgs = I.mixed_cfgs(grad_norm=False)
    assert not cfgs["grad_norm"].any()
    G, sq = gradient_and_sumsq(build_guide(case, cfgs=cfgs), case["joints"], case["start"], case["goal"], I.T_CHECK)
    G0, sq0 = gradient_and_sumsq(build_guide(case, cfgs=I.mixed_cfgs(False, grad_norm=False)), case["joints"], case["start"], case["goal"], I.T_CHECK)
    want = math.fsum((G.astype(np.float64) ** 2).ravel().tolist())
    rel = abs(sq - want) / want
    record(test="rowsq", case=name, rel_err=rel, bound=8 * 2.0 ** -24)
    assert rel <= 8 * 2.0 ** -24, (sq, want)
    rows = list(I.SELF_ROWS)
    others = [r for r in range(B) if r not in rows]
    assert np.array_equal(G[others], G0[others]) and not np.array_equal(G[rows], G0[rows]) and sq != sq0


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
    assert float(np.abs(out["clearance"] - bare["clearance"]).max()) <= max(R.GATE_FACTOR * float(np.abs(e32["clearance"] - ev["clearance"]).max()),
                                                                              R.GATE_FLOOR * ev["coord_max"])


# ---- runs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_net():
    from edmp_amd import weights as W
    from edmp_amd.temporalunet import TemporalUNet

    return TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=W.init_state_dict(5, 7, 32, TINY_DIMS), max_batch=64)


def with_102(guides):
    return [102 if n == 101 else n for n in guides]


def test_scene_batch_equals_serial_runs(tiny_net):
    """3. three scenes with guide 102 at different places (beside guide 13, whose rows normalise by the scene's ||g||): 24 guided steps of
    the batch equal each scene's serial run bit for bit - raw gradient, sum g^2 and the normalising neighbours all enter the state - and so
    does the report"""
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch

    parts = SI.scene_parts()
    S, Bs, N = SI.S, SI.B, SI.N
    cfgs = [SI.cfgs_for(with_102(p["guides"]), Bs // len(p["guides"])) for p in parts]
    plain = [SI.cfgs_for(p["guides"], Bs // len(p["guides"])) for p in parts]
    assert all(c["sdf_self_weight"].any() and "sdf_self_weight" not in q for c, q in zip(cfgs, plain))
    mk = lambda cs: [IntersectionVolumeGuide(p["obstacle_config"], DEV, cs[s], Bs, obstacle_kinds=p["kinds"]) for s, p in enumerate(parts)]  # noqa: E731
    guides, guides0 = mk(cfgs), mk(plain)
    starts, goals = np.stack([p["start"] for p in parts]), np.stack([p["goal"] for p in parts])
    noises = SI.noises()
    dif, t_stop = Diffusion(T, DEV), T - 24
    serial = lambda gs: [dif.denoise_guided(tiny_net, g, N, 7, g._sched, batch_size=Bs, start=starts[s], goal=goals[s], noise=noises[s], t_stop=t_stop)  # noqa: E731
                         for s, g in enumerate(gs)]
    ref, ref0 = serial(guides), serial(guides0)
    batch = SceneBatch(guides)
    assert batch.has_self_term
    got = dif.denoise_guided_scenes(tiny_net, batch, N, 7, starts, goals, noise=noises, t_stop=t_stop)
    for s in range(S):
        assert np.isfinite(ref[s]).all() and np.array_equal(got[s], ref[s]), s
        assert not np.array_equal(ref[s], ref0[s]), s  # the term moves the weighted rows
    gn = np.flatnonzero(cfgs[1]["grad_norm"])
    assert gn.size and not np.array_equal(ref[1][gn], ref0[1][gn])  # and, through the norm, their normalising neighbours
    for t in (0, R.T_CHECK):
        rep = batch.sdf_self_rows(got, t)
        for s in range(S):
            one = guides[s].sdf_self_rows(got[s][:, :, 1:-1], t)
            assert np.array_equal(rep["cost"][s], one["cost"]) and np.array_equal(rep["clearance"][s], one["clearance"]), (t, s)
    # position independence: scene 1 alone in a batch of one
    alone = dif.denoise_guided_scenes(tiny_net, SceneBatch([guides[1]]), N, 7, starts[1:2], goals[1:2], noise=[noises[1]], t_stop=t_stop)
    assert np.array_equal(alone[0], ref[1])


def run_cfgs():
    from edmp_amd import guide_cfg as GC

    return GC.build_guide_cfgs([GC.load_guide_dict(n) for n in (1, 102, 13)], 4, T)


def test_device_loop_equals_the_stepwise_api(tiny_net):
    """4. six steps (three of them guided) of the device loop against edmp_step_a_dev / edmp_step_b_dev, guide 102 beside a normalising one"""
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion, guided_step
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = run_cfgs()
    Bn = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, Bn)
    assert guide.has_self_term
    dif = Diffusion(T, DEV)
    noise = noise_for(4, Bn)
    s, gl = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    n = 6
    assert sum(guided_step(t) for t in range(T, T - n, -1)) >= 1
    X_loop = dif.denoise_guided(tiny_net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=Bn, start=s, goal=gl, noise=noise, t_stop=T - n)
    X = noise[0].copy()
    X[:, :, 0], X[:, :, -1] = s, gl
    for k, t in enumerate(range(T, T - n, -1)):
        X = dif.denoise_step(tiny_net, guide, X, noise[1 + k], t, s, gl, cfgs["guidance_schedule"])["x_out"]
    assert np.array_equal(X_loop, X)


def test_full_run_with_guide_102(tiny_net):
    """5. all 255 steps with guide 102 between guides 1 and 13: finite, bit-identical when repeated, not the run of guide 101, and a
    report that leaves a segmented run running"""
    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = run_cfgs()
    Bn = cfgs["total_batch_size"]
    scene, s, gl = scenes.random_scene(7, 8), scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    noise = noise_for(4, Bn)
    dif = Diffusion(T, DEV)

    def run(c):
        guide = IntersectionVolumeGuide(scene, DEV, c, Bn)
        return dif.denoise_guided(tiny_net, guide, 50, 7, c["guidance_schedule"], batch_size=Bn, start=s, goal=gl, noise=noise), guide

    X1, guide = run(cfgs)
    X2, _ = run(cfgs)
    assert np.isfinite(X1).all() and np.array_equal(X1, X2)
    X101, _ = run(GC.build_guide_cfgs([GC.load_guide_dict(n) for n in (1, 101, 13)], 4, T))
    assert not np.array_equal(X1[4:8], X101[4:8])
    assert np.array_equal(X1[:4], X101[:4])  # guide 1 does not normalise: its rows do not see the term
    rep = guide.sdf_self_rows(X1[:, :, 1:-1], 0)
    assert np.isfinite(rep["cost"]).all() and np.isfinite(rep["clearance"]).all()


def test_refusals():
    """6. every misuse is an error return whose message names the entry point, and the bound state is what it was"""
    from edmp_amd import _capi
    from edmp_amd.guide import SceneBatch

    case = I.check_case("L2_default")
    cfgs = case["cfgs"]
    plain = build_guide(case, cfgs={k: v for k, v in I.mixed_cfgs(False).items() if k not in SI.SDF_KEYS})
    plain._bind()
    lib, h = plain.ctx.lib, plain.ctx.h
    mask = np.ascontiguousarray(case["mask"].astype(np.int32).reshape(81))
    w, m = np.ascontiguousarray(cfgs["sdf_self_weight"]), np.ascontiguousarray(cfgs["sdf_self_margin"])

    def call(mask_=mask, w_=w, m_=m, n=B, T_=T):
        rc = lib.edmp_sdf_set_self(h, _capi.as_pi32(mask_), _capi.as_pd(np.ascontiguousarray(w_)), _capi.as_pd(np.ascontiguousarray(m_)), n, T_)
        return rc, (lib.edmp_last_error() or b"").decode()

    rc, msg = call()  # before edmp_sdf_set
    assert rc == -3 and msg.startswith("edmp_sdf_set_self") and "edmp_sdf_set" in msg, (rc, msg)
    guide = build_guide(case)
    guide._bind()
    before = guide.sdf_self_rows(case["joints"], I.T_CHECK)
    G = guide.get_gradient(case["joints"], case["start"], case["goal"], I.T_CHECK)
    w_bad = w.copy()
    w_bad[3] = 1.0  # an iv row
    bad_mask = mask.copy()
    bad_mask[0 * 9 + 5] = 2
    for what, kw, needle in (("wrong n", dict(n=B - 1), "rows"), ("wrong T", dict(T_=T - 1), "steps"), ("weight on a non-SDF row", dict(w_=w_bad), "row 3"),
                             ("negative margin", dict(m_=-m - 1.0), "self_margin"), ("NaN weight", dict(w_=np.full(B, np.nan)), "weight"),
                             ("mask entry 2", dict(mask_=bad_mask), "pair_mask")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("edmp_sdf_set_self") and needle in msg, (what, rc, msg)
    after = guide.sdf_self_rows(case["joints"], I.T_CHECK)
    assert np.array_equal(after["cost"], before["cost"]) and np.array_equal(after["clearance"], before["clearance"])
    assert np.array_equal(guide.get_gradient(case["joints"], case["start"], case["goal"], I.T_CHECK), G)
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_self_rows_dev"):
        guide.sdf_self_rows(case["joints"][:3], I.T_CHECK)  # t >= 1 reads the rows' schedules
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_self_rows_dev"):
        guide.sdf_self_rows(np.zeros((2, 7, 63)), 0)
    # a later edmp_sdf_set drops the term: the gradient is that of the ensemble without it, and the report asks for the table again
    guide._term_on["self"] = False
    guide._set_sdf()
    G0 = build_guide(case, cfgs=I.mixed_cfgs(False)).get_gradient(case["joints"], case["start"], case["goal"], I.T_CHECK)
    guide._bind()
    assert np.array_equal(guide.get_gradient(case["joints"], case["start"], case["goal"], I.T_CHECK), G0)
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
    batch = SceneBatch([a, build_guide(case, bind=False)])
    batch._bind()
    w2 = np.concatenate([w, w_bad])
    rc = lib.edmp_sdf_set_self(h, _capi.as_pi32(mask), _capi.as_pd(w2), _capi.as_pd(np.ascontiguousarray(np.concatenate([m, m]))), 2 * B, T)
    msg = (lib.edmp_last_error() or b"").decode()
    assert rc == -1 and "scene 1, row 3" in msg, (rc, msg)
