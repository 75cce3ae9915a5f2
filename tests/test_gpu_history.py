"""GPU: results do not depend on what a context ran before.

A context keeps a great deal between calls by design ("State a context keeps between calls"): recycled device blocks that are
handed out without clearing, guide scratch that only grows, UNet activation buffers sized for max_batch, a sampler with sticky switches
and leftovers, resident model / guide slots.  Every other GPU test asks "is this call right?" on objects built a moment earlier; this
module asks "is it still right after the context has done other work?" - through the public surface only (the Python objects and the
C ABI behind `ctx.lib`), by making real earlier calls.

A PROBE is a fixed list of calls with fixed seeded inputs that returns a dict of host arrays (keys "<item>/<array>", items unet, guide,
loop, check, fwd).  A HISTORY is a list of other calls made first on the same context and the same model / guide / Diffusion objects.
The property: the probe's arrays are bit-identical under every history - `_same_bits` compares the raw bits (NaN pattern included), no
tolerance anywhere.  So that "identically wrong five times" cannot pass, the probe without history also meets the gates the suite
applies to the same kind of call against the oracle (numbers copied unchanged from the tests named beside them).

Every arm lives on its own `runtime.Context(0)`, closed in a `finally`; one or two contexts are open at a time.  A new context is not
clean memory (hipMalloc may return pages a closed context just freed), hence "all histories agree" and not "equals the fresh run" alone.

How H-larger makes the probe receive the blocks it dirtied.  The pool (ctx_alloc / ctx_release) is keyed by rounded size, first
released first taken among equal sizes.
* `kind` (<= 64 int32) is always a 256-byte block.  A new guide object takes two 256-byte blocks from the pool: `sumsq`, then `kind`.
  The probe's success-check guide (`arm.check`, all cuboids) is evicted from its slot during the history, so the probe builds it
  again: its `sumsq` is the first free 256-byte block, its `kind` the second.  hl_nine_more_guides makes sure free ones exist: nine
  4-row guides that own eight 256-byte blocks each (row_class, method, grad_norm, rowsq, sumsq, vol_rows, kind, flags) are evicted
  by nine 80-row guides that take two each (sumsq, kind: their row arrays are 512- and 768-byte blocks), which leaves some thirty
  free.  hl_mark_free_blocks, the history's last step, then re-sets the scene of a CYLINDER guide with the probe's obstacle count
  192 times on one slot and marks the cylinders each time: every edmp_scene_set puts the slot's `kind` block behind the free
  256-byte blocks and takes the one in front, edmp_scene_set_shapes writes ones into it, so after more re-sets than there are free
  blocks every free 256-byte block starts with cylinder marks - the two the rebuilt check guide takes among them.  Only the
  memset in edmp_scene_set makes that guide's obstacles cuboids again; without it check/* differs (9 of the 12 seeded rows change
  their first colliding waypoint when the obstacles are cylinders).
* the probe's guide object itself (`arm.guide`) is evicted too, then bound again by the history and used at L = 62, so the probe's
  L = 5 and L = 48 calls run inside scratch shaped for 62 waypoints (capacity != shape), while under H-none capacity and shape coincide.
* the scene batch leaves four other start / goal pairs in the sampler, `condition=False` is the last loop call before the probe.

Replaced history steps: "a scene batch in the same guide slot" - the Python surface gives a SceneBatch its own slot and a per-scene
entry point on a batch-bound slot is refused, so the batch runs in its own slot of the same context (the nearest accepted call).
"The cylinder guide dropped so that its blocks return to the pool": a guide leaves a context only by eviction, so it is dropped by the
eighteen guides bound after it; hl_mark_free_blocks builds the same object again in a fresh slot for the marking, and that one stays
resident while the probe runs (what the probe's guide receives are the FREE blocks).

The segmented run (edmp_denoise_guided_segment_dev / edmp_denoise_scenes_segment_dev) keeps track of where it stands: see
`test_segmented_run_*` and include/edmp_hip.h.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.util import (FULL_DIMS, T, TINY_DIMS, cfgs_for, f64_error_ratio, host_metrics, maxabs, metrics_gate, noise_for, noisy_lines,
                        rmse)

pytestmark = pytest.mark.gpu

PB = 12                                   # rows of the probe's guides: [1, 10, 11, 18, 9, 13] x 2
P_GUIDES = [1, 10, 11, 18, 9, 13]
NO = 7                                    # obstacles of the probe's scenes (and of the history's cylinder scene)
ERR_ARG, ERR_STATE = -1, -3


# ---- fixed inputs ------------------------------------------------------------------------------------------------------------
def _inputs():
    from edmp_amd import scenes
    from oracle import edmp_oracle as O

    rs = np.random.RandomState(20)
    lo, hi = O.joint_limits()
    d = dict(lo=lo, hi=hi)
    d["x37"] = torch.tensor(rs.standard_normal((37, 7, 50)) * 1.5, dtype=torch.float32)
    d["x1"] = torch.tensor(rs.standard_normal((1, 7, 50)) * 1.5, dtype=torch.float32)
    d["x3"] = torch.tensor(rs.standard_normal((3, 7, 50)) * 1.5, dtype=torch.float32)
    d["scene"] = scenes.random_scene(47, NO)
    d["check_scene"] = scenes.random_scene(50, NO)  # (treated as cylinders, 9 of the 12 `rows` below change their first colliding waypoint)
    d["cfgs"] = cfgs_for(P_GUIDES, 2)
    d["start"], d["goal"] = scenes.random_start_goal(3)
    d["q"] = {L: O.clip_joints(rs.uniform(lo[None, :, None], hi[None, :, None], (PB, 7, L))) for L in (5, 48)}
    d["traj"] = O.clip_joints(rs.uniform(lo[None, :, None], hi[None, :, None], (PB, 7, 50)))
    r2 = np.random.RandomState(200)  # straight joint-space lines inside the limits: some rows free, some colliding on the way
    a, b, w = r2.uniform(lo * 0.8, hi * 0.8, (PB, 7)), r2.uniform(lo * 0.8, hi * 0.8, (PB, 7)), np.linspace(0, 1, 50)
    d["rows"] = np.ascontiguousarray(a[:, :, None] * (1 - w) + b[:, :, None] * w)
    d["noise"] = noise_for(5, PB)
    d["x0"] = rs.standard_normal((5, 7, 50))
    d["q_eps"] = rs.standard_normal((5, 7, 50))
    d["q_t"] = np.array([1, 255, 128, 7, 64])
    return d


@pytest.fixture(scope="module")
def inp():
    return _inputs()


@pytest.fixture(scope="module")
def sds():
    from edmp_amd import weights as W

    return W.init_state_dict(11, 7, 32, FULL_DIMS), W.init_state_dict(5, 7, 32, TINY_DIMS)


class Arm:
    """one context with the probe's objects: FULL net (max_batch 130), TINY net (max_batch 64), the probe's guide, the all-cuboid
    success-check guide and the T = 255 diffuser"""

    def __init__(self, inp, sds):
        from edmp_amd.diffusion import Diffusion
        from edmp_amd.guide import IntersectionVolumeGuide
        from edmp_amd.runtime import Context
        from edmp_amd.temporalunet import TemporalUNet

        self.inp = inp
        self.ctx = Context(0)
        try:
            self.full = TemporalUNet(None, 7, 32, self.ctx, dims=FULL_DIMS, state_dict=sds[0], max_batch=130)
            self.tiny = TemporalUNet(None, 7, 32, self.ctx, dims=TINY_DIMS, state_dict=sds[1], max_batch=64)
            self.guide = IntersectionVolumeGuide(inp["scene"], self.ctx, inp["cfgs"], PB)
            self.check = IntersectionVolumeGuide(inp["check_scene"], self.ctx, inp["cfgs"], PB)
            self.dif = Diffusion(T, self.ctx)
        except BaseException:
            self.ctx.close()
            raise
        self.keep = []   # history objects stay alive (and resident, until evicted) while the probe runs
        self.loop = None

    def close(self):
        self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ---- the probe ---------------------------------------------------------------------------------------------------------------
TAPS = list(range(6)) + [100] + [200 + j for j in range(5)]


def p_unet(arm):
    """FULL forward at B = 37 and B = 1 (t = 123) with every readable tap, the TINY model used in between and after"""
    from edmp_amd import _capi

    i, out = arm.inp, {}
    t = torch.tensor([123.0])
    for tag, x in (("37", i["x37"]), ("1", i["x1"])):
        out[f"unet/eps{tag}"] = arm.full(x, t).cpu().numpy()
        for w in TAPS:
            try:
                out[f"unet/tap{w}_{tag}"] = arm.full.activation(w, x.shape[0]).cpu().numpy()
            except _capi.EdmpError as e:
                # levels merged into one launch have no copy in device memory (test_gpu_parity.test_unet_golden): only those three
                assert "no activation tap" in str(e) and w in (0, 203, 204), (w, str(e))
        out[f"unet/tiny3_after{tag}"] = arm.tiny(i["x3"], torch.tensor([40.0])).cpu().numpy()
    return out


def p_guide(arm):
    """cost, swept-volume cost and gradient at L = 5 then L = 48, t = 128 and t = 6; per-row swept volumes and their arg-min"""
    i, g, out = arm.inp, arm.guide, {}
    for L in (5, 48):
        q = i["q"][L]
        for t in (128, 6):
            out[f"guide/cost_L{L}_t{t}"] = g.cost(torch.tensor(q), t).cpu().numpy()
            out[f"guide/swept_L{L}_t{t}"] = g.swept_volume_cost(torch.tensor(q), i["start"], i["goal"], t).cpu().numpy()
            out[f"guide/grad_L{L}_t{t}"] = g.get_gradient(q, i["start"], i["goal"], t)
    v, k = g.row_swept_volumes(i["start"], i["goal"], i["traj"])
    out["guide/row_volumes"], out["guide/argmin"] = v, np.array([k])
    return out


def p_loop(arm):
    """255 steps at B = 12 on the TINY net: guided with explicit noise, the same unguided, guided with device noise, and the guided run
    again through the chunked NumPy-stream path (np.random.seed(5) is the stream of noise_for(5, .))"""
    i, out = arm.inp, {}
    kw = dict(batch_size=PB, start=i["start"], goal=i["goal"])
    sch = i["cfgs"]["guidance_schedule"]
    out["loop/guided"] = arm.dif.denoise_guided(arm.tiny, arm.guide, 50, 7, sch, noise=i["noise"], **kw)
    out["loop/unguided"] = arm.dif.denoise_guided(arm.tiny, None, 50, 7, None, noise=i["noise"], **kw)
    out["loop/device"] = arm.dif.denoise_guided(arm.tiny, arm.guide, 50, 7, sch, noise="device", seed=3, **kw)
    np.random.seed(5)
    out["loop/chunked"] = arm.dif.denoise_guided(arm.tiny, arm.guide, 50, 7, sch, **kw)
    arm.loop = out
    return out


def p_check(arm):
    """the success check on the loop's outputs and on seeded in-limit rows against the all-cuboid scene (flags in the caller's arrays,
    then in the guide's own flag block with the four counters), metrics at N = 50, and the row choice"""
    from edmp_amd import _capi, franka
    from edmp_amd.runtime import ptr

    i, g, out = arm.inp, arm.check, {}
    loop = arm.loop or p_loop(arm)
    for tag, X in (("guided", loop["loop/guided"]), ("unguided", loop["loop/unguided"]), ("rows", i["rows"])):
        r = g.success_rows(X)
        out[f"check/ok_{tag}"], out[f"check/first_{tag}"], out[f"check/within_{tag}"] = r["ok"], r["first"], r["within"]
        out[f"check/counts_{tag}"] = np.array([r["rows_ok"], r["rows_within"], r["rows_collision_free"], r["rows"]])
    ctx = arm.ctx
    g._bind()
    Xd = ctx.to_dev(i["rows"], torch.float64)
    counts = (C.c_int32 * 4)()
    dh = np.ascontiguousarray(franka.dh_table_f64())
    _capi.check(ctx.lib.edmp_success_rows_dev(ctx.h, ptr(Xd), PB, 50, 4, _capi.as_pd(dh), None, None, None, counts), "edmp_success_rows_dev")
    out["check/counts_own_flags"] = np.array(list(counts))
    m = g.metrics_rows(loop["loop/unguided"])
    for k in m:
        out[f"check/metric_{k}"] = m[k]
    k0, vols, _ = g.select_row(i["start"], i["goal"], i["rows"])
    k1, vols1, m1 = g.select_row(i["start"], i["goal"], i["rows"], prefer="shortest")
    out["check/select"], out["check/select_volumes"] = np.array([k0, k1]), np.stack([vols, vols1])
    out["check/select_metric"] = m1["joint_path_length"]
    return out


def p_fwd(arm):
    i = arm.inp
    xt, mean, _ = arm.dif.q_sample(i["x0"], i["q_t"], i["q_eps"])
    return {"fwd/xt": xt, "fwd/mean": mean}


PROBE = dict(unet=p_unet, guide=p_guide, loop=p_loop, check=p_check, fwd=p_fwd)


def probe(arm):
    out = {}
    for fn in PROBE.values():
        out.update(fn(arm))
    return out


# ---- histories ---------------------------------------------------------------------------------------------------------------
def _uniform_q(seed, B, L, inp):
    from oracle import edmp_oracle as O

    rs = np.random.RandomState(seed)
    return O.clip_joints(rs.uniform(inp["lo"][None, :, None], inp["hi"][None, :, None], (B, 7, L)))


def hl_forwards(arm):
    rs = np.random.RandomState(31)
    arm.full(torch.tensor(rs.standard_normal((130, 7, 50)) * 1.5, dtype=torch.float32), torch.tensor([123.0]))
    arm.tiny(torch.tensor(rs.standard_normal((64, 7, 50)) * 1.5, dtype=torch.float32), torch.tensor([40.0]))


def hl_big_guide(arm):
    """64 obstacles, all 16 shipped guide classes x 3 rows, cost and gradient at L = 62"""
    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = cfgs_for(sorted(GC.GUIDE_CATALOG), 3)
    B = cfgs["total_batch_size"]
    g = IntersectionVolumeGuide(scenes.random_scene(3, 64), arm.ctx, cfgs, B)
    arm.keep.append(g)
    q = _uniform_q(32, B, 62, arm.inp)
    s, e = scenes.random_start_goal(9)
    g.cost(torch.tensor(q), 100)
    assert np.isfinite(g.get_gradient(q, s, e, 100)).all()
    g.row_swept_volumes(s, e, _uniform_q(33, B, 64, arm.inp))


def hl_scene_batch(arm):
    """S = 4 scenes (3, 7, 16, 64 obstacles) x 12 rows, four different start / goal pairs, 60 guided steps in one launch chain"""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch

    gs = [IntersectionVolumeGuide(scenes.random_scene(60 + k, no), arm.ctx, arm.inp["cfgs"], PB) for k, no in enumerate((3, 7, 16, 64))]
    sg = [scenes.random_start_goal(40 + k) for k in range(4)]
    batch = SceneBatch(gs)
    arm.keep += gs + [batch]
    rs = np.random.RandomState(34)
    X = arm.dif.denoise_guided_scenes(arm.tiny, batch, 50, 7, np.stack([a for a, _ in sg]), np.stack([b for _, b in sg]),
                                      noise=[rs.standard_normal((T + 1, PB, 7, 50)) for _ in range(4)], t_stop=T - 60)
    assert np.isfinite(X).all()


def hl_graph_and_device_noise(arm):
    from edmp_amd import scenes

    i = arm.inp
    s, e = scenes.random_start_goal(50)
    nz = arm.ctx.to_dev(noise_for(35, PB), torch.float64)
    run = lambda: arm.dif.denoise_guided(arm.tiny, arm.guide, 50, 7, i["cfgs"]["guidance_schedule"], batch_size=PB, start=s, goal=e, noise=nz, t_stop=T - 30)  # noqa: E731
    arm.dif.set_graph_replay(True)
    try:
        a = run()  # capture
        b = run()  # replay
    finally:
        arm.dif.set_graph_replay(False)
    assert np.array_equal(a, b)
    arm.dif.denoise_guided(arm.tiny, arm.guide, 50, 7, i["cfgs"]["guidance_schedule"], batch_size=PB, start=s, goal=e, noise="device", seed=99, t_stop=T - 30)


def hl_other_T_then_unconditioned(arm):
    """a second Diffusion(T = 50) on the context used once, then the T = 255 object again with condition=False: the LAST loop call of
    the history (a probe run that did not set the switch itself would come out unconditioned)"""
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion

    rs = np.random.RandomState(36)
    s, e = scenes.random_start_goal(51)
    d50 = Diffusion(50, arm.ctx)
    d50.denoise_guided(arm.tiny, None, 50, 7, None, batch_size=20, start=s, goal=e, noise=rs.standard_normal((51, 20, 7, 50)))
    X = arm.dif.denoise_guided(arm.tiny, None, 50, 7, None, batch_size=20, start=s, goal=e, condition=False, noise=rs.standard_normal((T + 1, 20, 7, 50)), t_stop=T - 40)
    assert not np.allclose(X[:, :, 0], s)


def hl_fwd_and_metrics(arm):
    from edmp_amd.evaluation import metrics_rows_on

    rs = np.random.RandomState(37)
    arm.dif.q_sample(rs.standard_normal((64, 7, 50)), rs.randint(1, T + 1, 64), rs.standard_normal((64, 7, 50)))
    metrics_rows_on(arm.ctx, noisy_lines(1024, 129, seed=3))


def _cylinder_guide(arm, B):
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    return IntersectionVolumeGuide(scenes.random_scene(70, NO), arm.ctx, cfgs_for([1, 10], B // 2), B, obstacle_kinds=np.ones(NO, dtype=np.int32))


def hl_cylinders(arm):
    """a scene of true cylinders with the probe's obstacle count, success check on 24 rows (more than the probe's)"""
    g = _cylinder_guide(arm, 24)
    arm.keep.append(g)
    arm.cyl = g
    assert g.success_rows(_uniform_q(38, 24, 50, arm.inp))["rows"] == 24


def hl_nine_more_guides(arm):
    """beyond the 8 guide slots of a context: the probe's two guides (and most of the history's) are evicted, their blocks go to the pool.
    Nine guides of 4 rows that use every small array a guide can own (five tables, two scratch arrays, the flags: eight 256-byte
    blocks each), then nine guides of 80 rows (whose row arrays are larger: two 256-byte blocks each) that evict them - which leaves
    some thirty 256-byte blocks free in the pool, so that the guide the probe rebuilds is served from blocks that were free, and
    marked, before (hl_mark_free_blocks)."""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    i = arm.inp
    cfgs = cfgs_for([1, 10], 2)
    for k in range(9):
        g = IntersectionVolumeGuide(scenes.random_scene(80 + k, 3), arm.ctx, cfgs, 4)
        g.cost(torch.tensor(_uniform_q(39 + k, 4, 48, i)), 0)
        g.get_gradient(_uniform_q(139 + k, 4, 48, i), i["start"], i["goal"], 100)
        g.success_rows(_uniform_q(239 + k, 4, 50, i))
        arm.keep.append(g)
    cfgs = cfgs_for([1, 10], 40)
    for k in range(9):
        g = IntersectionVolumeGuide(scenes.random_scene(180 + k, 3), arm.ctx, cfgs, 80)
        g.cost(torch.tensor(_uniform_q(339 + k, 2, 48, i)), 0, batch_size=2)
        arm.keep.append(g)


def hl_probe_guide_at_62(arm):
    """the probe's guide object, rebuilt after its eviction, at the largest L: its scratch is shaped for 62 waypoints from here on"""
    i = arm.inp
    q = _uniform_q(49, PB, 62, i)
    arm.guide.cost(torch.tensor(q), 100)
    assert np.isfinite(arm.guide.get_gradient(q, i["start"], i["goal"], 100)).all()
    arm.guide.row_swept_volumes(i["start"], i["goal"], _uniform_q(50, PB, 64, i))


def hl_mark_free_blocks(arm):
    """see the module docstring: the cylinder scene re-set 192 times on its slot, cylinders marked each time, then checked once more"""
    from edmp_amd import _capi

    g, ctx = arm.cyl, arm.ctx
    g._bind()
    ones = np.ones(NO, dtype=np.int32)
    for _ in range(192):
        _capi.check(ctx.lib.edmp_scene_set(ctx.h, _capi.as_pd(g.obstacle_config), NO, _capi.as_pd(g._cls_clr), _capi.as_pd(g._cls_exp), g._cls_clr.shape[0],
                                           g.T, _capi.as_pf(g._half), _capi.as_pf(g._dh), _capi.as_pf(g._sf)), "edmp_scene_set")
        _capi.check(ctx.lib.edmp_scene_set_shapes(ctx.h, _capi.as_pi32(ones), NO), "edmp_scene_set_shapes")
    assert g.success_rows(_uniform_q(38, 24, 50, arm.inp))["rows"] == 24


def hs_minimum(arm):
    """every dimension at its minimum, so that the probe is the call that grows each scratch buffer"""
    from edmp_amd import scenes
    from edmp_amd.evaluation import metrics_rows_on
    from edmp_amd.guide import IntersectionVolumeGuide

    i = arm.inp
    one = torch.tensor([123.0])
    arm.full(i["x1"] * 0.5, one)
    arm.tiny(i["x3"][:1], one)
    cfgs = cfgs_for([1], 1)
    g = IntersectionVolumeGuide(scenes.random_scene(90, 1), arm.ctx, cfgs, 1)
    arm.keep.append(g)
    s, e = scenes.random_start_goal(52)
    g.cost(torch.tensor(_uniform_q(53, 1, 1, i)), 6)
    g.get_gradient(_uniform_q(54, 1, 2, i), s, e, 6)
    g.row_swept_volumes(s, e, _uniform_q(55, 1, 3, i))
    g.success_rows(_uniform_q(56, 1, 2, i))
    rs = np.random.RandomState(57)
    arm.dif.denoise_guided(arm.tiny, g, 50, 7, cfgs["guidance_schedule"], batch_size=1, start=s, goal=e, noise=rs.standard_normal((T + 1, 1, 7, 50)), t_stop=T - 6)
    arm.dif.denoise_guided(arm.tiny, g, 50, 7, cfgs["guidance_schedule"], batch_size=1, start=s, goal=e, noise="device", seed=1, t_stop=T - 6)
    # the probe's own guide objects at the smallest shapes their rows allow
    arm.guide.cost(torch.tensor(_uniform_q(58, PB, 1, i)), 6)
    arm.guide.get_gradient(_uniform_q(59, PB, 2, i), s, e, 6)
    arm.check.success_rows(_uniform_q(60, 1, 2, i))
    metrics_rows_on(arm.ctx, _uniform_q(61, 1, 3, i))
    arm.dif.q_sample(rs.standard_normal((1, 7, 50)), np.array([9]), rs.standard_normal((1, 7, 50)))


def hn_nonfinite(arm):
    """Non-finite values only through kernels whose addressing does not depend on data: the UNet's convolution / GroupNorm / Mish
    kernels index by (sample, channel, position) alone, edmp_metrics_rows_dev is covered by test_non_finite_rows, and
    edmp_psample_dev is one element per thread.  After the forwards every activation buffer of both models holds NaN in rows
    0..max_batch-1, so a tail tile of the probe's B = 37 forward that read past its clamp shows as NaN, not as a last-bit difference.
    Nothing non-finite goes into the guide's cost / gradient kernels, the success check or the device loop."""
    from edmp_amd.evaluation import metrics_rows_on

    t = torch.tensor([123.0])
    for net, mb in ((arm.full, 130), (arm.tiny, 64)):
        assert torch.isnan(net(torch.full((mb, 7, 50), float("nan")), t)).all().item()
        x = torch.full((mb, 7, 50), 3e38)
        x[:, ::2] = -3e38
        net(x, t)  # (squares and sums of +-3e38 overflow inside: Inf and Inf - Inf in the GroupNorm statistics)
        assert torch.isnan(net(torch.full((mb, 7, 50), float("nan")), t)).all().item()  # NaN, not Inf, is what stays behind
    X = noisy_lines(64, 50)
    X[5, 3, 20], X[40, 0, 7] = np.nan, np.inf
    metrics_rows_on(arm.ctx, X)
    rs = np.random.RandomState(62)
    z = rs.standard_normal((4, 7, 50))
    z[1, 2, 3] = np.nan
    out = arm.dif.p_sample_using_posterior(rs.standard_normal((4, 7, 50)), 100, rs.standard_normal((4, 7, 50)).astype(np.float32), z=z)
    assert np.isnan(out[1, 2, 3]) and np.count_nonzero(np.isnan(out)) == 1


def h_self(arm):
    probe(arm)


HISTORIES = {
    "none": [],
    # loop calls first, condition=False the last of them; then the guides: cylinders, evictions, the probe's guide at L = 62, and the
    # marking of the pool's free blocks as the very last step
    "larger": [hl_forwards, hl_big_guide, hl_scene_batch, hl_graph_and_device_noise, hl_other_T_then_unconditioned, hl_fwd_and_metrics, hl_cylinders,
               hl_nine_more_guides, hl_probe_guide_at_62, hl_mark_free_blocks],
    "smaller": [hs_minimum],
    "nonfinite": [hn_nonfinite],
    "self": [h_self],
}
# per history and probe item: (rows, last-axis indices) the history's calls touched in that item's buffers; None = all of them
TOUCHED_BOUND = {
    "larger": dict(unet=(130, 50), guide=(48, 62), loop=(48, 50), check=(24, 50), fwd=(64, 50)),
    "smaller": dict(unet=(1, 50), guide=(12, 2), loop=(1, 50), check=(1, 3), fwd=(1, 50)),
    "nonfinite": dict(unet=(130, 50), guide=(0, 0), loop=(4, 50), check=(64, 50), fwd=(0, 0)),
}
TOUCHED = {
    "larger": "UNet rows 0..129 (FULL) / 0..63 (TINY), guide scratch up to 48 rows x 62 waypoints, 4 start/goal pairs, flags for 24 rows, q_sample 64 rows",
    "smaller": "row 0 and waypoints 0..1 only",
    "nonfinite": "NaN in UNet rows 0..129 (FULL) / 0..63 (TINY) of every activation buffer",
    "self": "exactly the probe's own rows and waypoints",
}


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a.astype(np.int64) if a.dtype.kind in "bui" else a


def _same_bits(name, a, b, ha, hb, fails):
    if a.shape != b.shape or a.dtype != b.dtype:
        fails.append(f"{name}: {a.dtype}{a.shape} after H-{ha}, {b.dtype}{b.shape} after H-{hb}")
        return
    d = _bits(a) != _bits(b)
    if d.any():
        idx = np.argwhere(d)
        rows = sorted(set(idx[:, 0].tolist())) if a.ndim > 1 else []
        last = (int(idx[:, -1].min()), int(idx[:, -1].max()))
        first = tuple(idx[0].tolist())
        bound = TOUCHED_BOUND.get(hb, {}).get(name.split("/")[0])
        inside = True if bound is None else bool(idx[:, 0].max() < bound[0] and (a.ndim < 2 or idx[:, -1].max() < bound[1]))
        fails.append(f"{name}: {int(d.sum())} of {d.size} elements differ between H-{ha} and H-{hb}; first at {first} ({a[first]!r} vs {b[first]!r}); "
                     f"rows {rows[:12]}{'...' if len(rows) > 12 else ''}, last-axis indices {last[0]}..{last[1]}, NaN {int(np.isnan(a).sum()) if a.dtype.kind == 'f' else 0} vs "
                     f"{int(np.isnan(b).sum()) if b.dtype.kind == 'f' else 0}; all inside the rows / waypoints H-{hb} touched: {'yes' if inside else 'NO'} "
                     f"({TOUCHED.get(hb, 'everything')})")


def _compare(ra, rb, ha, hb, items=None):
    fails = []
    if items is None and set(ra) != set(rb):
        fails.append(f"probe arrays differ in kind: {sorted(set(ra) ^ set(rb))}")
    for k in sorted(set(ra) & set(rb)):
        if items is None or k.split("/")[0] in items:
            _same_bits(k, ra[k], rb[k], ha, hb, fails)
    return fails


@pytest.fixture(scope="module")
def baseline(inp, sds):
    """the probe on a context without history (H-none)"""
    with Arm(inp, sds) as arm:
        return probe(arm)


@pytest.mark.parametrize("history", [h for h in HISTORIES if h != "none"])
def test_probe_is_bit_identical_after_history(inp, sds, baseline, history):
    """assertion 1: every probe array under this history equals H-none's bit for bit (so all five histories agree)"""
    with Arm(inp, sds) as arm:
        for step in HISTORIES[history]:
            step(arm)
        arm.loop = None
        got = probe(arm)
    fails = _compare(baseline, got, "none", history)
    assert not fails, "\n".join(fails)


def test_probe_without_history_meets_the_suite_gates(inp, sds, baseline):
    """assertion 2: H-none's results against the float32 oracle and its float64 evaluation, with the gates of the tests named here"""
    from oracle import edmp_oracle as O
    from oracle import success_oracle as SO

    r, i = baseline, inp
    # eps (test_gpu_archs.test_architecture_vs_oracle): rmse <= 2e-5 s, max <= 2e-4 s, <= 3 x torch-float32's float64 error
    sd32 = {k: torch.from_numpy(v) for k, v in sds[0].items()}
    sd64 = {k: v.double() for k, v in sd32.items()}
    for tag, x in (("37", i["x37"]), ("1", i["x1"])):
        with torch.no_grad():
            y32 = O.unet_forward(sd32, x, torch.tensor([123.0])).numpy()
            y64 = O.unet_forward(sd64, x.double(), torch.tensor([123.0], dtype=torch.float64)).numpy()
        tr = {}
        with torch.no_grad():
            O.unet_forward(sd32, x, torch.tensor([123.0]), trace=tr)
        for w in TAPS:  # every readable tap: max <= 5e-4 max(1, max|ref| / 8) (test_gpu_archs)
            if f"unet/tap{w}_{tag}" in r:
                ref = tr["mid" if w == 100 else f"down{w}" if w < 100 else f"up{w - 200}"].numpy()
                a = r[f"unet/tap{w}_{tag}"]
                assert a.shape == ref.shape and maxabs(a, ref) <= 5e-4 * max(1.0, float(np.abs(ref).max()) / 8), (tag, w, maxabs(a, ref))
        assert sum(f"unet/tap{w}_{tag}" in r for w in TAPS) >= len(TAPS) - 3, tag
        eps = r[f"unet/eps{tag}"]
        s = max(1.0, float(np.sqrt(np.mean(y32 ** 2))))
        q = f64_error_ratio(eps, y32, y64)
        print(f"[history] eps B={tag}: rmse {rmse(eps, y32):.3e} max {maxabs(eps, y32):.3e} (scale {s:.3g}), f64 error x{q:.2f} torch-f32's")
        assert rmse(eps, y32) <= 2e-5 * s and maxabs(eps, y32) <= 2e-4 * s and q <= 3.0, (tag, rmse(eps, y32), maxabs(eps, y32), q)
    with torch.no_grad():
        y3 = O.unet_forward({k: torch.from_numpy(v) for k, v in sds[1].items()}, i["x3"], torch.tensor([40.0])).numpy()
    for tag in ("37", "1"):
        assert rmse(r[f"unet/tiny3_after{tag}"], y3) <= 2e-5, tag
    # costs 2e-6, gradient max <= 5e-5 / rmse <= 5e-6 with the reference's NaN pattern, swept volumes 2e-5 and the same arg-min
    # (test_gpu_parity.test_guide_edge_sizes_vs_oracle)
    og = O.GuideOracle(i["scene"], i["cfgs"], PB)
    for L in (5, 48):
        q32 = torch.tensor(i["q"][L], dtype=torch.float32)
        for t in (128, 6):
            assert maxabs(r[f"guide/cost_L{L}_t{t}"], og.cost(q32, t).numpy()) <= 2e-6, (L, t)
            ref = og.swept_volume_cost(q32, torch.tensor(i["start"], dtype=torch.float32), torch.tensor(i["goal"], dtype=torch.float32), t).numpy()
            assert maxabs(r[f"guide/swept_L{L}_t{t}"], ref) <= 2e-6, (L, t)
            a, b = r[f"guide/grad_L{L}_t{t}"], og.get_gradient(i["q"][L], i["start"], i["goal"], t)
            assert np.array_equal(np.isnan(a), np.isnan(b)), (L, t)
            fin = ~np.isnan(b)
            assert fin.any() and maxabs(a[fin], b[fin]) <= 5e-5 and rmse(a[fin], b[fin]) <= 5e-6, (L, t, maxabs(a[fin], b[fin]), rmse(a[fin], b[fin]))
    vb = np.asarray(og.row_swept_volumes(i["start"], i["goal"], i["traj"]))
    assert maxabs(r["guide/row_volumes"], vb) <= 2e-5 and int(r["guide/argmin"][0]) == int(np.argmin(vb))
    # the loop: chunked stream == resident stream bit for bit (test_chunked_numpy_stream_equals_resident_stream), unguided tracks the
    # oracle to 1e-4 (test_free_running_unguided), conditioning pins the ends (test_condition_false)
    assert np.array_equal(r["loop/chunked"], r["loop/guided"])

    class NoGuide:
        def get_gradient(self, q, s, g, t):
            return np.zeros_like(q)

    Xo = O.denoise_guided(O.UNetOracle(sds[1]), NoGuide(), T, 50, 7, np.zeros((PB, T)), PB, i["start"], i["goal"], noise=i["noise"])
    assert rmse(r["loop/unguided"], Xo) <= 1e-4, rmse(r["loop/unguided"], Xo)
    for k in ("guided", "unguided", "device"):
        X = r[f"loop/{k}"]
        assert np.isfinite(X).all() and np.array_equal(X[:, :, 0], np.broadcast_to(i["start"], (PB, 7))) and np.array_equal(X[:, :, -1], np.broadcast_to(i["goal"], (PB, 7))), k
    assert not np.array_equal(r["loop/guided"], r["loop/unguided"]) and not np.array_equal(r["loop/guided"], r["loop/device"])
    # success flags equal to the checker's (test_gpu_success), the counters equal to the flags' sums
    n_hit = 0
    for tag, X in (("guided", r["loop/guided"]), ("unguided", r["loop/unguided"]), ("rows", i["rows"])):
        ref = SO.success_rows(X, i["check_scene"])
        for k in ("ok", "first", "within"):
            assert np.array_equal(r[f"check/{k}_{tag}"], ref[k]), (tag, k)
        want = [int(ref["ok"].sum()), int(ref["within"].sum()), int((ref["first"] < 0).sum()), PB]
        assert r[f"check/counts_{tag}"].tolist() == want, (tag, r[f"check/counts_{tag}"], want)
        n_hit += int((ref["first"] >= 0).sum())
    assert r["check/counts_own_flags"].tolist() == r["check/counts_rows"].tolist()
    assert n_hit > 0, "the check scene touches no row: the probe would not see its obstacles' shapes"
    # metrics <= 1e-9 of the host functions (test_gpu_batch_metrics), the row choice is the first arg-min / the shortest near-minimal row
    dev = {k[len("check/metric_"):]: v for k, v in r.items() if k.startswith("check/metric_")}
    metrics_gate(dev, host_metrics(r["loop/unguided"], 0.1), r["loop/unguided"], 0.1, "history probe", max_excluded=0)
    vols = r["check/select_volumes"][0]
    assert int(r["check/select"][0]) == int(np.argmin(vols)) and np.array_equal(vols, r["check/select_volumes"][1])
    pl = host_metrics(i["rows"], 0.1)["joint_path_length"]
    cand = np.flatnonzero(vols.astype(np.float64) <= float(vols.min()) + 0.0008)
    assert int(r["check/select"][1]) == int(cand[np.argmin(pl[cand])])
    # q_sample: NumPy's evaluation bit for bit (test_forward_process_golden)
    al = np.asarray(O.schedule(T)[1])
    sa, sb = np.sqrt(al[i["q_t"] - 1])[:, None, None], np.sqrt(1 - al[i["q_t"] - 1])[:, None, None]
    assert np.array_equal(r["fwd/mean"], sa * i["x0"]) and np.array_equal(r["fwd/xt"], sa * i["x0"] + sb * i["q_eps"])


def _rc_msg(fn, *args):
    from edmp_amd import _capi

    rc = fn(*args)
    return rc, _capi.load().edmp_last_error().decode()


def test_refusals_leave_no_trace(inp, sds, baseline):
    """assertion 3: after each refused call the next probe item still equals H-none's.  The refusals are those that return AFTER touching
    state: a loop whose B is not the bound rows' (refused by the first guided step, after X_T, the start / goal pair and the first
    unguided step were enqueued), a guide whose rows are refused after its scene was built in a new slot (the probe's guide parked, a
    half-built object left in the current slot), per-scene entry points on a bound scene batch (the batch's slot stays current), a
    continuing segment that does not match the run; and those that must touch nothing: L > 62, substeps > 64, B > max_batch, t = 0."""
    from edmp_amd import _capi, scenes
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch
    from edmp_amd.runtime import ptr

    fails = []
    with Arm(inp, sds) as arm:
        ctx, lib, pd = arm.ctx, arm.ctx.lib, _capi.as_pd

        def after(what, items):
            arm.loop = None
            for it in items:
                fails.extend(f"after '{what}': {f}" for f in _compare(baseline, PROBE[it](arm), "none", "refusal", items=[it]))

        s2, e2 = (np.ascontiguousarray(v) for v in scenes.random_start_goal(77))
        # 1. wrong B through the loop's entry point: 5 rows against the guide's 12
        arm.tiny._bind(), arm.guide._bind()
        ctx.ensure_sampler(T)
        nz = ctx.to_dev(noise_for(41, 5), torch.float64)
        out = ctx.empty((5, 7, 50), torch.float64)
        rc, msg = _rc_msg(lib.edmp_denoise_guided_dev, ctx.h, ptr(nz), 5, pd(s2), pd(e2), 1, 0, 1, ptr(out))
        assert rc == ERR_ARG and "rows set" in msg, (rc, msg)
        ctx.sync()
        after("loop with B = 5 on a guide of 12 rows", ["loop", "guide"])
        # 2. a continuing segment that does not match the run in progress
        rc, msg = _rc_msg(lib.edmp_denoise_guided_segment_dev, ctx.h, ptr(nz), PB, pd(s2), pd(e2), 1, 100, 90, 0, 1, None)
        assert rc == ERR_STATE, (rc, msg)
        after("continuing segment without a run", ["loop"])
        # 3. a guide whose rows are refused: scene built in a fresh slot, rows refused
        bad = dict(inp["cfgs"])
        bad["guidance_method"] = np.where(np.arange(PB) == 3, 0.5, np.asarray(inp["cfgs"]["guidance_method"]))
        with pytest.raises(_capi.EdmpError, match="guidance_method"):
            IntersectionVolumeGuide(scenes.random_scene(5, 9), ctx, bad, PB)
        after("guide with a refused guidance_method", ["guide", "check"])
        # 4. per-scene entry points on a bound scene batch
        batch = SceneBatch([arm.guide, arm.check])
        q = ctx.to_dev(inp["q"][48], torch.float64)
        g_out = ctx.empty((PB, 7, 48), torch.float64)
        rc, msg = _rc_msg(lib.edmp_guide_gradient_dev, ctx.h, ptr(q), PB, 48, pd(s2), pd(e2), 10, ptr(g_out), None)
        assert rc == ERR_STATE and "scene batch" in msg, (rc, msg)
        nz12 = ctx.to_dev(inp["noise"], torch.float64)
        o12 = ctx.empty((PB, 7, 50), torch.float64)
        rc, msg = _rc_msg(lib.edmp_denoise_guided_dev, ctx.h, ptr(nz12), PB, pd(s2), pd(e2), 1, 0, 1, ptr(o12))
        assert rc == ERR_STATE and "scene batch" in msg, (rc, msg)
        rc, msg = _rc_msg(lib.edmp_success_rows_dev, ctx.h, ptr(o12), PB, 50, 4, None, None, None, None, None)
        assert rc == ERR_STATE and "scene batch" in msg, (rc, msg)
        after("per-scene entry points on a bound scene batch", ["guide", "loop", "check"])
        del batch
        # 5. shapes beyond the limits
        arm.guide._bind()
        q63 = ctx.to_dev(_uniform_q(42, PB, 63, inp), torch.float64)
        g63 = ctx.empty((PB, 7, 63), torch.float64)
        rc, msg = _rc_msg(lib.edmp_guide_gradient_dev, ctx.h, ptr(q63), PB, 63, pd(s2), pd(e2), 10, ptr(g63), None)
        assert rc == ERR_ARG and "62" in msg, (rc, msg)
        after("gradient at L = 63", ["guide"])
        with pytest.raises(_capi.EdmpError):
            arm.check.success_rows(inp["rows"], substeps=65)
        after("success check with 65 substeps", ["check"])
        with pytest.raises(_capi.EdmpError, match="max_batch"):
            arm.full(torch.zeros(131, 7, 50), torch.tensor([123.0]))
        with pytest.raises(_capi.EdmpError, match="outside 1"):
            arm.full(inp["x37"] * 3, torch.tensor([256.0]))
        after("forward with B = 131 and with t = 256", ["unet"])
        with pytest.raises(_capi.EdmpError, match="outside 1"):
            arm.dif.q_sample(np.ones((9, 7, 50)), np.array([3, 4, 5, 6, 7, 8, 9, 10, 0]), np.ones((9, 7, 50)))
        after("q_sample with t = 0 in row 8", ["fwd"])
        # and the whole probe once more at the end
        arm.loop = None
        fails.extend(_compare(baseline, probe(arm), "none", "all refusals"))
    assert not fails, "\n".join(fails)


# ---- the segmented run keeps track of where it stands -------------------------------------------------------------------------
class _SegRig:
    """a context with the TINY net, S per-scene guides of 12 rows (S = 1: the single-scene entry points; S = 3: the scene batch's), one
    resident noise stream and raw calls of the segment entry points"""

    def __init__(self, inp, sds, S):
        from edmp_amd import _capi, scenes
        from edmp_amd.diffusion import Diffusion
        from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch
        from edmp_amd.runtime import Context
        from edmp_amd.temporalunet import TemporalUNet

        self.S, self.B = S, S * PB
        self.ctx = Context(0)
        try:
            self.net = TemporalUNet(None, 7, 32, self.ctx, dims=TINY_DIMS, state_dict=sds[1], max_batch=64)
            self.guides = [IntersectionVolumeGuide(scenes.random_scene(100 + k, 4 + 3 * k), self.ctx, inp["cfgs"], PB) for k in range(S)]
            self.bound = SceneBatch(self.guides) if S > 1 else self.guides[0]
            self.spare = IntersectionVolumeGuide(scenes.random_scene(99, 5), self.ctx, inp["cfgs"], PB)
            self.dif = Diffusion(T, self.ctx)
            sg = [scenes.random_start_goal(110 + k) for k in range(S + 1)]
            self.starts = np.ascontiguousarray(np.stack([a for a, _ in sg[:S]]))
            self.goals = np.ascontiguousarray(np.stack([b for _, b in sg[:S]]))
            self.other = (np.ascontiguousarray(np.stack([sg[S][0]] * S)), np.ascontiguousarray(np.stack([sg[S][1]] * S)))
            self.noise = self.ctx.to_dev(np.random.RandomState(120 + S).standard_normal((T + 1, self.B, 7, 50)), torch.float64)
            self.ctx.sync()
        except BaseException:
            self.ctx.close()
            raise
        self.lib, self.pd = self.ctx.lib, _capi.as_pd

    def bind(self):
        from edmp_amd import _capi

        self.ctx.ensure_sampler(T)
        self.net._bind()
        self.bound._bind()
        _capi.check(self.lib.edmp_sampler_set_condition(self.ctx.h, 1))

    def _noise_at(self, t_hi, init):
        k = 0 if init else 1 + (T - t_hi)
        return C.c_void_p(self.noise.data_ptr() + k * self.B * 7 * 50 * 8)

    def seg(self, t_hi, t_lo, init, guided=1, out=None, sg=None):
        """(rc, message) of one segment call; sg = (starts, goals), default the run's own"""
        from edmp_amd.runtime import ptr

        s, g = sg if sg is not None else (self.starts, self.goals)
        o = ptr(out) if out is not None else None
        if self.S == 1:
            return _rc_msg(self.lib.edmp_denoise_guided_segment_dev, self.ctx.h, self._noise_at(t_hi, init), self.B, self.pd(s), self.pd(g), guided, t_hi, t_lo,
                           1 if init else 0, 1, o)
        return _rc_msg(self.lib.edmp_denoise_scenes_segment_dev, self.ctx.h, self._noise_at(t_hi, init), self.S, PB, self.pd(s), self.pd(g), guided, t_hi, t_lo,
                       1 if init else 0, 1, o)

    def whole(self, guided=1, sg=None):
        from edmp_amd import _capi
        from edmp_amd.runtime import ptr

        s, g = sg if sg is not None else (self.starts, self.goals)
        out = self.ctx.empty((self.B, 7, 50), torch.float64)
        if self.S == 1:
            rc = self.lib.edmp_denoise_guided_dev(self.ctx.h, ptr(self.noise), self.B, self.pd(s), self.pd(g), guided, 0, 1, ptr(out))
        else:
            rc = self.lib.edmp_denoise_scenes_dev(self.ctx.h, ptr(self.noise), self.S, PB, self.pd(s), self.pd(g), guided, 0, 1, ptr(out))
        _capi.check(rc, "whole run")
        return self.ctx.to_host(out)

    def sentinel(self):
        out = self.ctx.empty((self.B, 7, 50), torch.float64)
        with torch.cuda.stream(self.ctx.stream):
            out.fill_(float("nan"))
        return out

    def close(self):
        self.ctx.close()


CUTS = [(T, 200), (200, 128), (128, 7), (7, 0)]


@pytest.mark.parametrize("S", [1, 3])
def test_segmented_run_equals_the_whole_run(inp, sds, S):
    """the positive path: a run cut at {200, 128, 7} equals the unsegmented run bit for bit, one scene and S = 3, guided and unguided"""
    rig = _SegRig(inp, sds, S)
    try:
        rig.bind()
        for guided in (1, 0):
            want = rig.whole(guided)
            out = rig.sentinel()
            for k, (hi, lo) in enumerate(CUTS):
                rc, msg = rig.seg(hi, lo, init=(k == 0), guided=guided, out=out if lo == 0 else None)
                assert rc == 0, (guided, hi, lo, rc, msg)
            assert np.array_equal(rig.ctx.to_host(out), want), guided
        assert not np.array_equal(rig.whole(1), rig.whole(0))
    finally:
        rig.close()


@pytest.mark.parametrize("S", [1, 3])
def test_segmented_run_refuses_a_continuation_that_is_no_run(inp, sds, S):
    """A continuing segment (init == 0) is accepted only at the step the kept state stands at, on the context the run was started on.
    Refused with EDMP_ERR_STATE, nothing launched (the output keeps its sentinel): steps skipped or repeated (the message names the
    expected and the given step), a complete run or a teacher-forced step in between, another model / guide bound in between (the
    context's epoch moved), edmp_sampler_init in between, a changed conditioning switch, another batch size, and a run that already
    reached step 0; a forward of the bound model, or a gradient / swept-cost / row-volume call of the bound guide, in between (they replace
    the model's input buffer and the guide's start / goal pair, which the next segment reads); a guided continuation of a run that was
    started unguided.  A refusal for a wrong step leaves the run as it stands: the matching segment is then accepted and the run ends bit
    for bit where the unsegmented run ends.  start / goal of a continuing segment are ignored (include/edmp_hip.h): the run goes on
    with the init call's pair."""
    from edmp_amd import _capi
    from edmp_amd.temporalunet import TemporalUNet

    rig = _SegRig(inp, sds, S)
    try:
        rig.bind()
        want = rig.whole(1)
        out = rig.sentinel()

        def untouched():
            return torch.isnan(out).all().item()

        def start_run():
            rc, msg = rig.seg(T, 200, init=True)
            assert rc == 0, msg

        # steps skipped / repeated; the right step is still accepted afterwards and the other pair on the way is ignored
        start_run()
        for t_hi in (190, 210, T):
            rc, msg = rig.seg(t_hi, t_hi - 10, init=False, out=out)
            assert rc == ERR_STATE and "200" in msg and str(t_hi) in msg and untouched(), (t_hi, rc, msg)
        for hi, lo in CUTS[1:]:
            rc, msg = rig.seg(hi, lo, init=False, out=out if lo == 0 else None, sg=rig.other)
            assert rc == 0, (hi, lo, msg)
        assert np.array_equal(rig.ctx.to_host(out), want)
        # a run that reached step 0 is over
        out = rig.sentinel()
        rc, msg = rig.seg(7, 0, init=False, out=out)
        assert rc == ERR_STATE and "no run in progress" in msg and untouched(), (rc, msg)
        assert not np.array_equal(rig.whole(1, sg=rig.other), want)  # (the other pair does give another run when it is the init call's)
        # a complete run in between has overwritten the kept state
        start_run()
        rig.whole(1)
        rc, msg = rig.seg(200, 128, init=False, out=out)
        assert rc == ERR_STATE and "no run in progress" in msg and untouched(), (rc, msg)
        # the conditioning switch changed in between
        start_run()
        _capi.check(rig.lib.edmp_sampler_set_condition(rig.ctx.h, 0))
        _capi.check(rig.lib.edmp_sampler_set_condition(rig.ctx.h, 1))
        rc, msg = rig.seg(200, 128, init=False, out=out)
        assert rc == ERR_STATE and "no run in progress" in msg and untouched(), (rc, msg)
        # another batch size
        start_run()
        rc, msg = (_rc_msg(rig.lib.edmp_denoise_guided_segment_dev, rig.ctx.h, rig._noise_at(200, False), rig.B - 1, rig.pd(rig.starts), rig.pd(rig.goals), 0, 200, 128, 0, 1, None)
                   if S == 1 else
                   _rc_msg(rig.lib.edmp_denoise_scenes_segment_dev, rig.ctx.h, rig._noise_at(200, False), S, PB - 1, rig.pd(rig.starts), rig.pd(rig.goals), 0, 200, 128, 0, 1, None))
        assert rc == ERR_STATE and "no run in progress" in msg, (rc, msg)
        rc, msg = rig.seg(200, 128, init=False)  # (that refusal did not end the run either)
        assert rc == 0, msg
        # the sampler re-initialised with another T and back
        start_run()
        rig.ctx.ensure_sampler(50)
        rig.ctx.ensure_sampler(T)
        rc, msg = rig.seg(200, 128, init=False, out=out)
        assert rc == ERR_STATE and "no run in progress" in msg and untouched(), (rc, msg)
        # another model bound in between, the run's model bound again: the epoch moved
        other = TemporalUNet(None, 7, 32, rig.ctx, dims=TINY_DIMS, seed=9, max_batch=64)
        rig.bind()
        start_run()
        other._bind()
        rig.bind()
        rc, msg = rig.seg(200, 128, init=False, out=out)
        assert rc == ERR_STATE and "changed" in msg and "200" in msg and untouched(), (rc, msg)
        # another guide bound in between
        start_run()
        rig.spare._bind()
        rig.bind()
        rc, msg = rig.seg(200, 128, init=False, out=out)
        assert rc == ERR_STATE and "changed" in msg and untouched(), (rc, msg)
        # a teacher-forced step in between replaces the start / goal pair (single-scene entry point; refused on a batch before that)
        if S == 1:
            from edmp_amd.runtime import ptr

            start_run()
            Xd = rig.ctx.empty((rig.B, 7, 50), torch.float64)
            with torch.cuda.stream(rig.ctx.stream):
                Xd.zero_()
            _capi.check(rig.lib.edmp_step_b_dev(rig.ctx.h, ptr(Xd), rig.B, 9, rig.pd(rig.other[0]), rig.pd(rig.other[1]), None), "edmp_step_b_dev")
            rc, msg = rig.seg(200, 128, init=False, out=out)
            assert rc == ERR_STATE and "no run in progress" in msg and untouched(), (rc, msg)
        # a forward of the run's own model in between: the model's input buffer carried the next segment's input
        start_run()
        rig.net(inp["x3"], torch.tensor([40.0]))
        rc, msg = rig.seg(200, 128, init=False, out=out)
        assert rc == ERR_STATE and "no run in progress" in msg and untouched(), (rc, msg)
        # a run started unguided never gave the guide its start / goal pair: no guided continuation (the unguided one goes on)
        rc, msg = rig.seg(T, 200, init=True, guided=0)
        assert rc == 0, msg
        rc, msg = rig.seg(200, 128, init=False, guided=1, out=out)
        assert rc == ERR_STATE and "unguided" in msg and "200" in msg and untouched(), (rc, msg)
        rc, msg = rig.seg(200, 128, init=False, guided=0)
        assert rc == 0, msg
        # the guide's own entry points replace its start / goal pair (single scene; a bound batch refuses them before that)
        if S == 1:
            calls = [lambda: rig.bound.get_gradient(inp["q"][48], rig.other[0][0], rig.other[1][0], 100),
                     lambda: rig.bound.swept_volume_cost(torch.tensor(inp["q"][48]), rig.other[0][0], rig.other[1][0], 100),
                     lambda: rig.bound.row_swept_volumes(rig.other[0][0], rig.other[1][0], inp["traj"])]
            for k, call in enumerate(calls):
                start_run()
                call()
                rc, msg = rig.seg(200, 128, init=False, out=out)
                assert rc == ERR_STATE and "no run in progress" in msg and untouched(), (k, rc, msg)
        # and the context still runs: segmented and whole
        out2 = rig.sentinel()
        for k, (hi, lo) in enumerate(CUTS):
            rc, msg = rig.seg(hi, lo, init=(k == 0), out=out2 if lo == 0 else None)
            assert rc == 0, msg
        assert np.array_equal(rig.ctx.to_host(out2), want) and np.array_equal(rig.whole(1), want)
    finally:
        rig.close()
