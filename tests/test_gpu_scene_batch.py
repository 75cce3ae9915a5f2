"""Scene batches on the GPU: S scenes x B rows planned in ONE device-resident loop (Diffusion.denoise_guided_scenes over a
guide.SceneBatch) must give every scene exactly what its own serial denoise_guided run gives - bit for bit, under the same noise - and
the per-scene entry points must refuse a bound batch instead of answering with scene 0's data."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.util import FULL_DIMS, T, cfgs_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def net():
    from edmp_amd.temporalunet import TemporalUNet

    return TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, max_batch=3 * B)


@pytest.fixture(scope="module")
def dif():
    from edmp_amd.diffusion import Diffusion

    return Diffusion(T, DEV)


def _scenes():
    """three scenes with 4, 16 (3 true cylinders) and 64 obstacles, their own starts / goals and guide configs; together the configs
    hold iv, sv and grad_norm rows (guides 1, 5, 10, 11, 13)"""
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.scenes import SyntheticDataset

    spec = [(4, 0, ([1, 5, 10], 8)), (16, 3, ([11, 13], 12)), (64, 0, ([13, 1, 11, 5], 6))]
    guides, starts, goals = [], [], []
    for k, (no, ncyl, (gl, bpg)) in enumerate(spec):
        ds = SyntheticDataset(scene_types=("stress",), num_scenes_per_type=3, n_obstacles=no, n_cylinders=ncyl)
        oc, _, _, ncub, nc, start, ik = ds.fetch_data(scene_num=k, scene_type="stress")
        kinds = np.concatenate([np.zeros(int(ncub), dtype=np.int32), np.ones(int(nc), dtype=np.int32)])
        cfgs = cfgs_for(gl, bpg)
        assert cfgs["total_batch_size"] == B
        guides.append(IntersectionVolumeGuide(oc, DEV, cfgs, B, obstacle_kinds=kinds))
        starts.append(start)
        goals.append(ik[k])
    return guides, np.stack(starts), np.stack(goals)


@pytest.fixture(scope="module")
def scenes():
    return _scenes()


def _serial(dif, net, guides, starts, goals, noises, **kw):
    guided = kw.pop("guided", True)
    return [dif.denoise_guided(net, g if guided else None, 50, 7, g._sched, batch_size=B, start=starts[s], goal=goals[s], noise=noises[s], **kw)
            for s, g in enumerate(guides)]


@pytest.mark.parametrize("mode", ["full", "t_stop", "unguided", "graph", "pinned", "pinned_t_stop", "numpy_stream"])
def test_scene_batch_equals_serial_runs(net, dif, scenes, mode):
    from edmp_amd.guide import SceneBatch

    guides, starts, goals = scenes
    S = len(guides)
    batch = SceneBatch(guides)
    rs = np.random.RandomState(1000 + len(mode))
    noises = [rs.standard_normal((T + 1, B, 7, 50)) for _ in range(S)]
    kw, bkw = {}, {}
    if mode in ("t_stop", "pinned_t_stop"):
        kw = bkw = dict(t_stop=100)
    if mode == "unguided":
        kw, bkw = dict(guided=False), dict(guided=False)
    if mode == "numpy_stream":
        # noise=None: the S streams come from the global RandomState in scene order, as S serial calls draw them
        np.random.seed(4242)
        ref = [dif.denoise_guided(net, g, 50, 7, g._sched, batch_size=B, start=starts[s], goal=goals[s]) for s, g in enumerate(guides)]
        state_serial = np.random.get_state()
        np.random.seed(4242)
        got = dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals)
        state_batch = np.random.get_state()
        assert state_serial[0] == state_batch[0] and np.array_equal(state_serial[1], state_batch[1]) and state_serial[2:] == state_batch[2:]
    else:
        ref = _serial(dif, net, guides, starts, goals, noises, **kw)
        if mode == "graph":
            dif.set_graph_replay(True)
            try:
                first = dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals, noise=noises)
                got = dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals, noise=noises)  # the same call again: replayed
            finally:
                dif.set_graph_replay(False)
            assert np.array_equal(first, got)
        elif mode in ("pinned", "pinned_t_stop"):
            pinned = [torch.from_numpy(n).pin_memory() for n in noises]
            got = dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals, noise=pinned, chunk_steps=8, **bkw)
        else:
            got = dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals, noise=noises, **bkw)
    assert got.shape == (S, B, 7, 50)
    for s in range(S):
        assert np.array_equal(got[s], ref[s]), (mode, s)
    assert not np.array_equal(ref[0], ref[1])
    if mode in ("full", "numpy_stream"):
        # the per-scene guides still pick the best row and check success after the batch bound its own slot
        for s, g in enumerate(guides):
            v_b, i_b = g.row_swept_volumes(starts[s], goals[s], got[s])
            v_r, i_r = g.row_swept_volumes(starts[s], goals[s], ref[s])
            assert i_b == i_r and np.array_equal(v_b, v_r)
            ok_b, ok_r = g.success_rows(got[s]), g.success_rows(ref[s])
            for key in ("ok", "first", "within", "collision_free"):
                assert np.array_equal(ok_b[key], ok_r[key]), (s, key)


def test_scene_batch_at_size():
    """two scenes of 1024 rows each under the six-guide ensemble of config 3: both equal their serial runs"""
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch
    from edmp_amd.scenes import SyntheticDataset
    from edmp_amd.temporalunet import TemporalUNet

    rows = 1024
    cfgs = cfgs_for([1, 2, 3, 4, 5, 10], 170, rows_per_guide=[171, 171, 171, 171, 170, 170])
    ds = SyntheticDataset(scene_types=("tabletop", "stress"), num_scenes_per_type=1, n_obstacles=16, n_cylinders=3)
    guides, starts, goals = [], [], []
    for st in ("tabletop", "stress"):
        oc, _, _, _, _, start, ik = ds.fetch_data(scene_num=0, scene_type=st)
        guides.append(IntersectionVolumeGuide(oc, DEV, cfgs, rows))
        starts.append(start)
        goals.append(ik[0])
    big = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, max_batch=2 * rows)
    dif = Diffusion(T, DEV)
    rs = np.random.RandomState(5)
    noises = [rs.standard_normal((T + 1, rows, 7, 50)) for _ in range(2)]
    got = dif.denoise_guided_scenes(big, SceneBatch(guides), 50, 7, np.stack(starts), np.stack(goals), noise=noises)
    for s, g in enumerate(guides):
        ref = dif.denoise_guided(big, g, 50, 7, g._sched, batch_size=rows, start=starts[s], goal=goals[s], noise=noises[s])
        assert np.array_equal(got[s], ref), s


def test_infer_serial_scenes_per_launch():
    """the driver planning two scenes per launch (five scenes: a leftover group of one) returns, scene by scene, what the serial loop
    returns under the same np.random seed, and leaves the global RandomState where the serial loop leaves it"""
    import infer_serial
    from edmp_amd import scenes

    cfg = os.path.join(ROOT, "configs", "cfg_c1_plumbing.yaml")
    out, states = [], []
    for k in (1, 2):
        np.random.seed(31)
        ds = scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=5, n_obstacles=6, n_cylinders=1)
        out.append(infer_serial.run(cfg, dataset=ds, verbose=False, scenes_per_launch=k))
        states.append(np.random.get_state())
    assert len(out[0]) == len(out[1]) == 5
    for a, b in zip(*out):
        assert (a["scene_num"], a["best_row"], a["success_proxy"], a["success_strict"], a["rows_ok"], a["rows_collision_free"]) == \
               (b["scene_num"], b["best_row"], b["success_proxy"], b["success_strict"], b["rows_ok"], b["rows_collision_free"])
        assert np.array_equal(a["trajectory"], b["trajectory"])
    assert [r["scenes_in_launch"] for r in out[1]] == [2, 2, 2, 2, 1]
    assert np.array_equal(states[0][1], states[1][1]) and states[0][2:] == states[1][2:]
    with pytest.raises(ValueError):
        infer_serial.run(cfg, verbose=False, scenes_per_launch=2, scenes_in_flight=2)


def _rc_msg(fn, *args):
    from edmp_amd import _capi

    rc = fn(*args)
    return rc, _capi.load().edmp_last_error().decode()


def test_refusals_on_a_bound_scene_batch(net, dif, scenes):
    from edmp_amd import _capi
    from edmp_amd.guide import SceneBatch
    from edmp_amd.runtime import ptr

    guides, starts, goals = scenes
    S = len(guides)
    batch = SceneBatch(guides)
    ctx = dif.ctx
    lib = ctx.lib
    ctx.ensure_sampler(T)
    net._bind()
    batch._bind()
    _capi.check(lib.edmp_sampler_set_condition(ctx.h, 1))
    noise = ctx.empty((T + 1, S * B, 7, 50), torch.float64)
    noise.zero_()
    out = ctx.empty((S * B, 7, 50), torch.float64)
    out.fill_(float("nan"))
    s0 = np.ascontiguousarray(starts[0], dtype=np.float64)
    g0 = np.ascontiguousarray(goals[0], dtype=np.float64)
    sa, ga = np.ascontiguousarray(starts, dtype=np.float64), np.ascontiguousarray(goals, dtype=np.float64)
    pd = _capi.as_pd
    ST, ARG = -3, -1
    # the single-scene loop, teacher-forced steps, cost, gradient, best trajectory and success on a bound batch
    cases = [
        (ST, "scene batch", lib.edmp_denoise_guided_dev, ctx.h, ptr(noise), S * B, pd(s0), pd(g0), 1, 0, 1, ptr(out)),
        (ST, "scene batch", lib.edmp_denoise_guided_segment_dev, ctx.h, ptr(noise), S * B, pd(s0), pd(g0), 1, T, T - 1, 1, 1, ptr(out)),
        (ST, "scene batch", lib.edmp_denoise_guided_rng_dev, ctx.h, 7, S * B, pd(s0), pd(g0), 1, 0, 1, ptr(out)),
        (ST, "scene batch", lib.edmp_step_a_dev, ctx.h, ptr(out), ptr(noise), S * B, 10, pd(s0), pd(g0), 1, None, None),
        (ST, "scene batch", lib.edmp_step_b_dev, ctx.h, ptr(out), S * B, 10, pd(s0), pd(g0), None),
        (ST, "scene batch", lib.edmp_guide_cost_dev, ctx.h, ptr(noise), S * B, 48, 0, 1, ptr(out)),
        (ST, "scene batch", lib.edmp_guide_gradient_dev, ctx.h, ptr(out), S * B, 48, pd(s0), pd(g0), 10, ptr(noise), None),
        (ST, "scene batch", lib.edmp_row_swept_volumes_dev, ctx.h, ptr(out), S * B, 50, pd(s0), pd(g0), ptr(noise), None),
        (ST, "scene batch", lib.edmp_success_rows_dev, ctx.h, ptr(out), S * B, 50, 4, None, None, None, None, None),
        # S or B out of range, scene count not the bound batch's, starts / goals missing while conditioning
        (ARG, "scenes outside", lib.edmp_denoise_scenes_dev, ctx.h, ptr(noise), 17, B, pd(sa), pd(ga), 1, 0, 1, ptr(out)),
        (ARG, "scenes outside", lib.edmp_denoise_scenes_dev, ctx.h, ptr(noise), 0, B, pd(sa), pd(ga), 1, 0, 1, ptr(out)),
        (ARG, "max_batch", lib.edmp_denoise_scenes_dev, ctx.h, ptr(noise), S, 4 * B, pd(sa), pd(ga), 1, 0, 1, ptr(out)),
        (ST, "holds 3 scene", lib.edmp_denoise_scenes_dev, ctx.h, ptr(noise), 2, B, pd(sa), pd(ga), 1, 0, 1, ptr(out)),
        (ARG, "required", lib.edmp_denoise_scenes_dev, ctx.h, ptr(noise), S, B, None, None, 1, 0, 1, ptr(out)),
        (ARG, "required", lib.edmp_denoise_scenes_segment_dev, ctx.h, ptr(noise), S, B, None, pd(ga), 0, T, T - 1, 1, 1, ptr(out)),
    ]
    for want, text, fn, *args in cases:
        rc, msg = _rc_msg(fn, *args)
        assert rc == want and text in msg, (fn.__name__, rc, msg)
    # an all-reduce hook installed (it sums ONE scalar)
    cb = _capi.ALLREDUCE_FN(lambda u, s, p: 0)
    _capi.check(lib.edmp_sampler_set_allreduce(ctx.h, C.cast(cb, C.c_void_p), None))
    try:
        rc, msg = _rc_msg(lib.edmp_denoise_scenes_dev, ctx.h, ptr(noise), S, B, pd(sa), pd(ga), 1, 0, 1, ptr(out))
    finally:
        _capi.check(lib.edmp_sampler_set_allreduce(ctx.h, None, None))
    assert rc == ST and "all-reduce hook" in msg, msg
    # rows that do not split over the scenes, rows of one scene on another scene's classes
    tb = batch.tables
    rc, msg = _rc_msg(lib.edmp_rows_set, ctx.h, _capi.as_pi32(tb["row_class"]), _capi.as_pf(tb["method"]), _capi.as_pd(tb["grad_norm"]),
                      _capi.as_pd(tb["guidance_schedule"]), S * B - 1, T)
    assert rc == ARG and "split evenly" in msg, msg
    rc_swapped = np.ascontiguousarray(tb["row_class"][::-1])
    rc, msg = _rc_msg(lib.edmp_rows_set, ctx.h, _capi.as_pi32(rc_swapped), _capi.as_pf(tb["method"]), _capi.as_pd(tb["grad_norm"]),
                      _capi.as_pd(tb["guidance_schedule"]), S * B, T)
    assert rc == ARG and "belongs to scene" in msg, msg
    # nothing was launched: the output still holds its sentinel
    assert torch.isnan(out).all().item()
    # the device noise mode through Python
    with pytest.raises(_capi.EdmpError, match="device noise"):
        dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals, noise="device")
    # and the batch still plans after every refusal
    X = dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals, noise=[np.zeros((T + 1, B, 7, 50))] * S)
    assert np.isfinite(X).all()
