"""The sphere signed-distance guide (edmp_amd/csrc/sdf.hip) on the GPU against its float64 checker (tests/sdf_reference.py).

Gate.  The kernel is f32, the checker f64.  Per case the checker's own formula is evaluated once more in float32 on the CPU; its largest
deviation from the float64 result, relative to the case's largest |gradient| element of the SDF rows (to the largest |cost| for the
cost), is the yardstick, and the kernel gets 4 x that (another summation order over spheres and links, the device's sinf / cosf), with a
floor of 4 f32 ulps of that largest element.  Every test prints the kernel's error, the yardstick and the gate; with
EDMP_SDF_PARITY_OUT=<file> the records are also written there as JSON (profiles/sdf_guide_parity.json comes from such a run).  The
inputs sit >= 1e-5 m away from every decision boundary of the cost (asserted by the checker's generator), so no element is excluded
from any comparison."""

import numpy as np
import pytest
import torch

from tests import sdf_reference as R
from tests import sdf_gpu
from tests.sdf_gpu import DEV, recorder, tiny_net  # noqa: F401  (tiny_net: this module's fixture)
from tests.util import noise_for

pytestmark = pytest.mark.gpu
T = R.T
VOLUME_GATE = 5e-5  # the suite's gate of the iv / sv raw gradient against the f32 oracle (test_gpu_parity.test_gradient_vs_oracle_random)


record, _write_records = recorder("sdf parity", "EDMP_SDF_PARITY_OUT", "max(4 x CPU-float32 deviation from float64, 4 f32 ulps), relative to the largest element")


def build_guide(case, cfgs=None, **kw):
    """sdf_gpu.build_guide; a case without a true cylinder hands no kinds over, and "custom" is the named case's sphere table"""
    custom = R.CASES[case["name"]]["spheres"] == "custom" if "name" in case else False
    return sdf_gpu.build_guide(dict(case, custom=custom), cfgs, obstacle_kinds=case["kinds"] if case["kinds"].any() else None, **kw)


def get_case(name):
    c = dict(R.check_case(name))
    c["name"] = name
    return c


def reference_mixed(case, chk_grad, joints, t, yardstick):
    """the mixed gradient (B, 7, L) the ensemble should return and a per-row absolute tolerance, from the references alone: the checker
    for the SDF rows, the suite's f32 oracle for the iv / sv rows, the whole-batch norm from both.
    Tolerances: an SDF row's raw gradient may miss by gs = gate x max |checker gradient|; a volume row's by VOLUME_GATE (the suite's
    own gate for that kernel).  The norm n = ||g_all|| then misses by at most dn = sqrt(n_sdf_elements) gs + sqrt(n_volume_elements)
    VOLUME_GATE (triangle inequality), and a normalised row g / n by (its raw tolerance + max |g_row| dn / n) / n."""
    from oracle import edmp_oracle as O

    cfgs, B = case["cfgs"], case["B"]
    raw = O.GuideOracle(case["obstacle_config"], R.mixed_cfgs(False), B).raw_gradient(joints, case["start"], case["goal"], t).astype(np.float64)
    sdf_rows = list(R.SDF_ROWS)
    raw[sdf_rows] = chk_grad[sdf_rows]
    gs = R.gate(yardstick["grad"]) * float(np.abs(chk_grad[sdf_rows]).max())
    n = float(np.sqrt((raw ** 2).sum()))
    per_row = raw[0].size
    dn = np.sqrt(len(sdf_rows) * per_row) * gs + np.sqrt((B - len(sdf_rows)) * per_row) * VOLUME_GATE
    gn = cfgs["grad_norm"]
    ref, tol = np.zeros_like(raw), np.zeros(B)
    for r in range(B):
        rt = gs if r in sdf_rows else VOLUME_GATE
        if gn[r]:
            ref[r] = raw[r] / n
            tol[r] = (rt + float(np.abs(raw[r]).max()) * dn / n) / n
        else:
            ref[r], tol[r] = raw[r], rt
    return ref, tol, gs, n


@pytest.mark.parametrize("t", [0, R.T_CHECK])
@pytest.mark.parametrize("name", list(R.CASES))
def test_cost_and_clearance_of_every_row(name, t):
    """1. sdf_rows against the checker at t = 0 (margin 0) and at a step with a non-constant margin schedule, every row of the batch"""
    case = get_case(name)
    guide = build_guide(case)
    ev = case["ev0"] if t == 0 else case["evt"]
    out = guide.sdf_rows(case["joints"], case["start"], case["goal"], t)
    y = R.f32_yardstick(case, t)
    cost_scale = float(np.abs(ev["cost"]).max())
    cost_err = float(np.abs(out["cost"] - ev["cost"]).max()) / cost_scale
    cgate, cy = R.case_clearance_gate(case, t)
    clr_err = float(np.abs(out["clearance"] - ev["clearance"]).max())
    record(test="cost_clearance", case=name, t=t, cost_rel_err=cost_err, cost_yardstick=y["cost"], cost_gate=R.gate(y["cost"]), clearance_abs_err=clr_err,
           clearance_yardstick_abs=cy, clearance_gate_abs=cgate)
    assert out["cost"].shape == (case["B"],) and out["cost"].dtype == np.float64
    assert cost_err <= R.gate(y["cost"]), (cost_err, y["cost"])
    assert clr_err <= cgate, (clr_err, cgate)
    if t == 0:  # any n at t = 0: the first rows alone (no smoothness weight then) equal the collision part
        sub = guide.sdf_rows(case["joints"][:2], case["start"], case["goal"], 0)
        assert float(np.abs(sub["cost"] - ev["collision"][:2]).max()) / cost_scale <= R.gate(y["cost"])
        assert np.array_equal(sub["clearance"], out["clearance"][:2])


@pytest.mark.parametrize("name", list(R.CASES))
def test_gradient_of_a_mixed_ensemble(name):
    """2. get_gradient on sdf / iv / sv rows with grad_norm 0 / 1: SDF rows against the checker, normalised rows against g / ||g_all|| with
    the norm from the references, and the iv / sv rows without normalisation BIT-identical to a guide built without any SDF guide"""
    case = get_case(name)
    t, ev = R.T_CHECK, case["evt"]
    y = R.f32_yardstick(case, t)
    G = build_guide(case).get_gradient(case["joints"], case["start"], case["goal"], t)
    G_again = build_guide(case).get_gradient(case["joints"], case["start"], case["goal"], t)
    G0 = build_guide(case, cfgs=R.mixed_cfgs(False)).get_gradient(case["joints"], case["start"], case["goal"], t)
    ref, tol, gs, n = reference_mixed(case, ev["grad"], case["joints"], t, y)
    scale = float(np.abs(ev["grad"][list(R.SDF_ROWS)]).max())
    err = [float(np.abs(G[r] - ref[r]).max()) for r in range(case["B"])]
    record(test="gradient", case=name, t=t, sdf_row_rel_err=err[0] / scale, yardstick=y["grad"], gate=R.gate(y["grad"]), row_abs_err=err, row_tolerance=tol.tolist(),
           norm=n, active_share=case["marginst"]["active"])
    assert G.shape == ev["grad"].shape and np.isfinite(G).all()
    assert np.array_equal(G, G_again)  # no atomics: bit-identical between runs
    for r in range(case["B"]):
        assert err[r] <= tol[r], (r, err[r], tol[r])
    for r in range(case["B"]):
        if r not in R.SDF_ROWS and not case["cfgs"]["grad_norm"][r]:
            assert np.array_equal(G[r], G0[r]), r


@pytest.mark.parametrize("L", [5, 48])
def test_smoothness_alone(L):
    """3. obstacles so far away that no hinge is active (asserted on the checker's d): the gradient is 2 lambda (2 q_w - q_{w-1} - q_{w+1})"""
    cfgs = R.mixed_cfgs()
    B = cfgs["total_batch_size"]
    inp = R.make_case(3, B, L, 3, 1, far=True)
    sph = R.case_spheres("default")
    m = cfgs["sdf_margin"][:, R.T_CHECK - 1]
    ev = R.evaluate(inp["joints"], inp["start"], inp["goal"], inp["obstacle_config"], inp["kinds"], sph, m, cfgs["smoothness"])
    assert float((ev["d"] - m.reshape(-1, 1, 1)).min()) > 1.0 and not ev["collision"].any()
    case = dict(inp, cfgs=cfgs, B=B, spheres=sph)
    G = build_guide(case).get_gradient(inp["joints"], inp["start"], inp["goal"], R.T_CHECK)
    lam = cfgs["smoothness"][0]
    assert lam > 0 and cfgs["smoothness"][1] == 0

    def closed(dtype):
        q = np.concatenate([inp["start"].reshape(7, 1), inp["joints"][0], inp["goal"].reshape(7, 1)], axis=1).astype(dtype)
        return (dtype(2) * dtype(lam) * (dtype(2) * q[:, 1:-1] - q[:, :-2] - q[:, 2:])).astype(np.float64)

    ref = closed(np.float64)
    scale = float(np.abs(ref).max())
    y = float(np.abs(closed(np.float32) - ref).max()) / scale
    err = float(np.abs(G[0] - ref).max()) / scale
    record(test="smoothness", L=L, rel_err=err, yardstick=y, gate=R.gate(y))
    assert err <= R.gate(y), (err, y)
    assert np.abs(G[0] - ev["grad"][0]).max() / scale <= R.gate(y)  # the checker says the same
    assert not G[1].any()  # the SDF row without smoothness weight has nothing to follow (g / ||g_all|| of zeros)


def test_teacher_forced_step(tiny_net):
    """4. one guided reverse step through edmp_step_a_dev / edmp_step_b_dev: the update of every row is sched x mixed, the mixed gradient
    being the references' at the clipped posterior state (SDF rows: the checker's), and the start / goal columns are pinned"""
    from edmp_amd.diffusion import Diffusion, guided_step
    from oracle import edmp_oracle as O

    case = get_case("L48_o7c2_custom")
    cfgs, B, t = case["cfgs"], case["B"], R.T_CHECK
    assert guided_step(t)
    guide = build_guide(case)
    X = np.concatenate([np.tile(case["start"].reshape(1, 7, 1), (B, 1, 1)), case["joints"], np.tile(case["goal"].reshape(1, 7, 1), (B, 1, 1))], axis=2)
    z = np.random.RandomState(21).standard_normal(X.shape)
    st = Diffusion(T, DEV).denoise_step(tiny_net, guide, X, z, t, case["start"], case["goal"], cfgs["guidance_schedule"])
    q = O.clip_joints(st["x_post"][:, :, 1:-1])
    # the guide sees start / goal as f32 (the kernels' start / goal pair)
    s32, g32 = case["start"].astype(np.float32).astype(np.float64), case["goal"].astype(np.float32).astype(np.float64)
    m = cfgs["sdf_margin"][:, t - 1]
    args = (q, s32, g32, case["obstacle_config"], case["kinds"], case["spheres"])
    ev = R.evaluate(*args, m, cfgs["smoothness"])
    rows = list(R.SDF_ROWS)
    evs = R.evaluate(q[rows], s32, g32, case["obstacle_config"], case["kinds"], case["spheres"], m[rows], cfgs["smoothness"][rows], want_grad=False)
    R.assert_margins(evs, "teacher-forced step, SDF rows")
    e32 = R.evaluate(*args, m, cfgs["smoothness"], dtype=torch.float32)
    y = dict(grad=float(np.abs(e32["grad"][rows] - ev["grad"][rows]).max() / np.abs(ev["grad"][rows]).max()))
    sub = dict(case, start=s32, goal=g32)
    ref, tol, gs, n = reference_mixed(sub, ev["grad"], q, t, y)
    sched = cfgs["guidance_schedule"][:, t - 1]
    upd = st["x_post"][:, :, 1:-1] - st["x_out"][:, :, 1:-1]
    err_g = [float(np.abs(st["grad"][r] - ref[r]).max()) for r in range(B)]
    err_u = [float(np.abs(upd[r] - sched[r] * ref[r]).max()) for r in range(B)]
    record(test="teacher_forced_step", t=t, yardstick=y["grad"], gate=R.gate(y["grad"]), grad_abs_err=err_g, update_abs_err=err_u, row_tolerance=tol.tolist())
    for r in range(B):
        assert err_g[r] <= tol[r], (r, err_g[r], tol[r])
        # x_out = x_post - sched * mixed in f64: beside the gradient's tolerance only the rounding of x itself (|x| < 4)
        assert err_u[r] <= sched[r] * tol[r] + 1e-15, (r, err_u[r])
    assert np.array_equal(st["x_out"][:, :, 0], np.tile(case["start"], (B, 1))) and np.array_equal(st["x_out"][:, :, -1], np.tile(case["goal"], (B, 1)))


def test_full_run_with_an_sdf_guide(tiny_net):
    """5. denoise_guided, B = 12, guide 101 between guides 1 and 10: finite, bit-identical across two runs; and with sdf_rows all zero the
    run is bit-identical to the run on a guide_cfgs without the SDF keys (nothing else is launched)"""
    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = GC.build_guide_cfgs([GC.load_guide_dict(n) for n in (1, 101, 10)], 4, T)
    B = cfgs["total_batch_size"]
    assert B == 12 and cfgs["sdf_rows"].sum() == 4
    scene = scenes.random_scene(7, 8)
    start, goal = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    noise = noise_for(4, B)
    dif = Diffusion(T, DEV)

    def run(c):
        guide = IntersectionVolumeGuide(scene, DEV, c, B)
        return dif.denoise_guided(tiny_net, guide, 50, 7, c["guidance_schedule"], batch_size=B, start=start, goal=goal, noise=noise), guide

    X1, guide = run(cfgs)
    X2, _ = run(cfgs)
    assert np.isfinite(X1).all() and np.array_equal(X1, X2)
    rep = guide.sdf_rows(X1[:, :, 1:-1], start, goal, 0)
    assert np.isfinite(rep["cost"]).all() and np.isfinite(rep["clearance"]).all()
    zero = dict(cfgs)
    zero["sdf_rows"] = np.zeros(B)
    plain = {k: v for k, v in cfgs.items() if k not in ("sdf_rows", "sdf_margin", "smoothness")}
    Xz, _ = run(zero)
    Xp, _ = run(plain)
    assert np.array_equal(Xz, Xp)
    assert not np.array_equal(X1[4:8], Xp[4:8])  # the SDF rows do take another path
    # guides 1 and 10 do not normalise: their rows do not see what the SDF rows do
    assert np.array_equal(X1[:4], Xp[:4]) and np.array_equal(X1[8:], Xp[8:])


def test_refusals():
    """6. every misuse is an error return with a message; nothing is launched"""
    from edmp_amd import _capi
    from edmp_amd.guide import SceneBatch

    case = get_case("L5_o7c2_default")
    cfgs, B = case["cfgs"], case["B"]
    guide = build_guide(case)
    guide._bind()
    lib, h = guide.ctx.lib, guide.ctx.h
    d = guide._sdf

    def call(spheres=None, n=None, B_=B, T_=T, rows=None, margin=None, smooth=None):
        sph = np.ascontiguousarray(d["spheres"] if spheres is None else spheres, dtype=np.float32)
        rc = lib.edmp_sdf_set(h, _capi.as_pf(sph), int(sph.shape[0] if n is None else n), _capi.as_pi32(d["rows"] if rows is None else rows),
                              _capi.as_pd(d["margin"] if margin is None else margin), _capi.as_pd(d["smooth"] if smooth is None else smooth), B_, T_)
        return rc, (lib.edmp_last_error() or b"").decode()

    def edited(i, j, v):
        s = d["spheres"].copy()
        s[i, j] = v
        return s

    assert call()[0] == 0
    for what, kw in (("wrong B", dict(B_=B - 1)), ("wrong T", dict(T_=T - 1)), ("link 9", dict(spheres=edited(0, 0, 9.0))), ("radius 0", dict(spheres=edited(1, 4, 0.0))),
                     ("too many spheres", dict(spheres=np.tile(d["spheres"][:1], (_capi.MAX_SPHERES + 1, 1)))), ("no spheres", dict(n=0)),
                     ("negative margin", dict(margin=np.full((B, T), -1.0))), ("NaN smoothness", dict(smooth=np.full(B, np.nan))),
                     ("sdf_row 2", dict(rows=np.full(B, 2, dtype=np.int32)))):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("edmp_sdf_set"), (what, rc, msg)
    # the table survives a refused call, and wrong row counts at t >= 1 are refused by the report as well
    out = guide.sdf_rows(case["joints"], case["start"], case["goal"], R.T_CHECK)
    assert np.isfinite(out["cost"]).all()
    with pytest.raises(_capi.EdmpError, match="edmp_sdf_rows_dev"):
        guide.sdf_rows(case["joints"][:3], case["start"], case["goal"], R.T_CHECK)
    # a bound scene batch refuses the table
    plain = build_guide(case, cfgs=R.mixed_cfgs(False), bind=False)
    batch = SceneBatch([plain, build_guide(case, cfgs=R.mixed_cfgs(False), bind=False)])
    batch._bind()
    z = np.zeros(2 * B)
    rc = lib.edmp_sdf_set(h, _capi.as_pf(d["spheres"]), int(d["spheres"].shape[0]), _capi.as_pi32(np.zeros(2 * B, dtype=np.int32)), _capi.as_pd(np.zeros((2 * B, T))),
                          _capi.as_pd(z), 2 * B, T)
    msg = (lib.edmp_last_error() or b"").decode()
    assert rc == -3 and "scene batch" in msg, (rc, msg)
    one = SceneBatch([plain])  # a batch of ONE scene is a batch too
    one._bind()
    rc = lib.edmp_sdf_set(h, _capi.as_pf(d["spheres"]), int(d["spheres"].shape[0]), _capi.as_pi32(np.zeros(B, dtype=np.int32)), _capi.as_pd(np.zeros((B, T))),
                          _capi.as_pd(np.zeros(B)), B, T)
    assert rc == -3, rc
