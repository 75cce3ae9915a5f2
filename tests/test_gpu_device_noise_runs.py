"""The device noise source (diffusion.DeviceNoise: Philox inside the step tail) in every run form: scene batches, warm starts, segments
and graph replay.  The stream contract: counter = (element, step, block, 0), key = seed, with the element index taken inside the row's
own scene and the key that scene's seed; step 0 = X_T of a full run or the eps of a re-noising warm start, 1 + T - t = reverse step t.

Every comparison is array_equal.  The references are the serial noise="device" path and the explicit-noise path fed the materialised
stream (Diffusion.device_noise); tests/test_device_noise.py holds both to oracle/device_rng.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.util import FULL_DIMS, T, cfgs_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ERR_STATE = -3
SEEDS3 = (2**32 + 7, 0, 2**64 - 1)
MAX_ROWS = 32


def _program_tail(net):
    """which kernel runs the step tail of the device-resident loop: the last op of the layer program decides"""
    net._bind()
    last = [n for n, _, _, _ in net.ctx.prof_ops()][-1]
    return "level" if last.startswith(("level_kernel<2,", "level2_kernel<1,")) else "psample"


@pytest.fixture(scope="module", params=["level", "psample"])
def net(request):
    """the full net in both programs: the tail inside the LV_UP_FINAL level kernel (default), or head_psample_kernel (EDMP_NO_LEVEL=1)"""
    from edmp_amd.temporalunet import TemporalUNet

    old = os.environ.get("EDMP_NO_LEVEL")
    if request.param == "psample":
        os.environ["EDMP_NO_LEVEL"] = "1"
    try:  # the builder reads its switches when the model is built
        n = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, seed=4, max_batch=MAX_ROWS)
        assert _program_tail(n) == request.param
    finally:
        if old is None:
            os.environ.pop("EDMP_NO_LEVEL", None)
        else:
            os.environ["EDMP_NO_LEVEL"] = old
    return n


@pytest.fixture(scope="module")
def dif():
    from edmp_amd.diffusion import Diffusion

    return Diffusion(T, DEV)


@pytest.fixture(scope="module")
def rig():
    """three scenes with 4, 7 and 10 obstacles, rows of guides 1 and 10 (three each), their own start / goal pairs"""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = cfgs_for([1, 10], 3)
    B = cfgs["total_batch_size"]
    assert (B * 50) % 64 != 0  # a scene boundary falls inside a wave and inside a level-kernel workgroup
    guides = [IntersectionVolumeGuide(scenes.random_scene(6 + k, n), DEV, cfgs, B) for k, n in enumerate((4, 7, 10))]
    starts = np.stack([scenes.DEFAULT_START + 0.01 * k for k in range(3)])
    goals = np.stack([scenes.DEFAULT_GOAL - 0.01 * k for k in range(3)])
    return dict(cfgs=cfgs, B=B, sched=cfgs["guidance_schedule"], guides=guides, starts=starts, goals=goals)


_DRAWS = {}


def _draw(dif, seed, k, B):
    """device_noise(seed, k, B), computed once and shared (read-only)"""
    key = (seed, k, B)
    if key not in _DRAWS:
        z = dif.device_noise(seed, k, B)
        z.setflags(write=False)
        _DRAWS[key] = z
    return _DRAWS[key]


def _stream(dif, seed, steps, B):
    return np.stack([_draw(dif, seed, k, B) for k in steps])


def _differs(a, b):
    return (float(np.abs(a - b).max()), np.argwhere(a != b)[:5].tolist())


# ---- 1. a scene batch equals its serial runs ------------------------------------------------------------------------------------
def test_scene_batch_equals_its_serial_device_runs(net, dif, rig):
    from edmp_amd.diffusion import DeviceNoise
    from edmp_amd.guide import SceneBatch

    B, S = rig["B"], 3
    batch = SceneBatch(rig["guides"])
    got = dif.denoise_guided_scenes(net, batch, 50, 7, rig["starts"], rig["goals"], noise=DeviceNoise(seeds=SEEDS3))
    assert got.shape == (S, B, 7, 50) and np.isfinite(got).all()
    for s, g in enumerate(rig["guides"]):
        ref = dif.denoise_guided(net, g, 50, 7, rig["sched"], batch_size=B, start=rig["starts"][s], goal=rig["goals"][s], noise="device", seed=SEEDS3[s])
        assert np.array_equal(got[s], ref), (s, _differs(got[s], ref))
        obj = dif.denoise_guided(net, g, 50, 7, rig["sched"], batch_size=B, start=rig["starts"][s], goal=rig["goals"][s], noise=DeviceNoise(SEEDS3[s]))
        assert np.array_equal(obj, ref), s  # the object form of a full single-scene run is the string form
    streams = [_stream(dif, SEEDS3[s], range(T + 1), B) for s in range(S)]
    fed = dif.denoise_guided_scenes(net, batch, 50, 7, rig["starts"], rig["goals"], noise=streams)
    assert np.array_equal(got, fed), _differs(got, fed)
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("rows", [1, 5])
def test_unguided_scene_batch_equals_its_serial_device_runs(net, dif, rows):
    """five scenes of 1 and of 5 rows, unguided (FINISH on every step), per-scene conditioning and Q3 on every scene's first row.

    An odd number of rows per scene puts every second scene at an odd row of the batch.  The level kernels take two (or four) rows per
    workgroup and sum a row's GroupNorm statistics in an order that depends on its slot there (one forward of the same input at an odd
    and at an even batch position differs by 1.1e-6), so they deal their workgroups scene by scene in a scene batch (level.hip: level_body):
    a row then sits in the slot it has in its scene's own run.  Without that the odd-numbered scenes here miss their serial runs by
    about 1e-6, under any noise source."""
    from edmp_amd import scenes
    from edmp_amd.diffusion import DeviceNoise
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch

    S = 5
    assert (rows * 50) % 64 != 0
    cfgs = cfgs_for([1], rows)
    assert cfgs["total_batch_size"] == rows
    batch = SceneBatch([IntersectionVolumeGuide(scenes.random_scene(30 + k, 4), DEV, cfgs, rows) for k in range(S)])
    starts = np.stack([scenes.DEFAULT_START + 0.02 * k for k in range(S)])
    goals = np.stack([scenes.DEFAULT_GOAL - 0.02 * k for k in range(S)])
    seeds = (5, 2**63, 5, 2**64 - 1, 1)  # equal seeds are allowed
    got = dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals, noise=DeviceNoise(seeds=seeds), guided=False)
    for s in range(S):
        ref = dif.denoise_guided(net, None, 50, 7, None, batch_size=rows, start=starts[s], goal=goals[s], noise="device", seed=seeds[s])
        assert np.array_equal(got[s], ref), (s, _differs(got[s], ref))
    one = dif.denoise(net, 50, 7, start=starts[0], goal=goals[0], batch_size=rows, noise=DeviceNoise(seeds[0]))
    assert np.array_equal(one, got[0][0] if rows == 1 else got[0])
    free = dif.denoise_guided_scenes(net, batch, 50, 7, None, None, noise=DeviceNoise(seeds=seeds), guided=False, condition=False)
    for s in (0, 4):
        ref = dif.denoise_guided(net, None, 50, 7, None, batch_size=rows, condition=False, noise="device", seed=seeds[s])
        assert np.array_equal(free[s], ref), s


# ---- 2. the element index is the scene's own --------------------------------------------------------------------------------------
def test_the_element_index_is_scene_local(net, dif, rig):
    from edmp_amd import scenes
    from edmp_amd.diffusion import DeviceNoise
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch

    B = rig["B"]
    twins = SceneBatch([IntersectionVolumeGuide(scenes.random_scene(6, 4), DEV, rig["cfgs"], B) for _ in range(2)])
    pair = np.stack([rig["starts"][0]] * 2), np.stack([rig["goals"][0]] * 2)
    same = dif.denoise_guided_scenes(net, twins, 50, 7, *pair, noise=DeviceNoise(seeds=(9, 9)), t_stop=T - 8)
    assert np.array_equal(same[0], same[1]), _differs(same[0], same[1])
    other = dif.denoise_guided_scenes(net, twins, 50, 7, *pair, noise=DeviceNoise(seeds=(9, 10)), t_stop=T - 8)
    assert np.array_equal(other[0], same[0]) and not np.array_equal(other[0], other[1])


# ---- 3. warm starts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_start", [32, T])
@pytest.mark.parametrize("n_scenes", [1, 3])
def test_warm_start_equals_the_explicit_run_fed_its_draws(net, dif, rig, n_scenes, t_start):
    """[step 0 when re-noising] + [steps T - t_start + 1 .. T - t_stop] of every scene's stream, fed to the explicit-noise warm run"""
    from edmp_amd.diffusion import DeviceNoise, WarmStart
    from edmp_amd.guide import SceneBatch

    B, S = rig["B"], n_scenes
    rs = np.random.RandomState(17)
    plans = {"group": rs.uniform(-1.0, 1.0, (S, 7, 50)), "row": rs.uniform(-1.0, 1.0, (S, B, 7, 50))}
    batch = SceneBatch(rig["guides"]) if S > 1 else None
    for t_stop in (0, 5):
        for renoise in (True, False):
            steps = ([0] if renoise else []) + list(range(T - t_start + 1, T - t_stop + 1))
            for per, x0 in plans.items():
                what = (S, t_start, t_stop, renoise, per)
                if S == 1:
                    g, kw = rig["guides"][0], dict(batch_size=B, start=rig["starts"][0], goal=rig["goals"][0], t_stop=t_stop)
                    ws = WarmStart(x0[0], t_start, renoise=renoise)
                    got = dif.denoise_guided(net, g, 50, 7, rig["sched"], noise=DeviceNoise(SEEDS3[0]), warm_start=ws, **kw)
                    ref = dif.denoise_guided(net, g, 50, 7, rig["sched"], noise=_stream(dif, SEEDS3[0], steps, B), warm_start=ws, **kw)
                else:
                    ws = WarmStart(x0, t_start, renoise=renoise)
                    got = dif.denoise_guided_scenes(net, batch, 50, 7, rig["starts"], rig["goals"], noise=DeviceNoise(seeds=SEEDS3), warm_start=ws, t_stop=t_stop)
                    ref = dif.denoise_guided_scenes(net, batch, 50, 7, rig["starts"], rig["goals"], noise=[_stream(dif, sd, steps, B) for sd in SEEDS3],
                                                    warm_start=ws, t_stop=t_stop)
                assert np.isfinite(got).all(), what
                assert np.array_equal(got, ref), (what, _differs(got, ref))


# ---- 4. - 6. through the C ABI ------------------------------------------------------------------------------------------------------
class _Abi:
    """the bound context of a single scene (S = 1) or of the three-scene batch, and the segment calls of both noise sources"""

    def __init__(self, net, dif, rig, S, seeds=None, guides=None):
        from edmp_amd import _capi
        from edmp_amd.guide import SceneBatch
        from edmp_amd.runtime import ptr

        self.ctx, self.lib, self.S, self.B, self.ptr = dif.ctx, dif.ctx.lib, S, rig["B"], ptr
        self.rows = S * self.B
        guides = rig["guides"][:S] if guides is None else guides
        if S == 1:
            dif._prepare(net, guides[0], self.B, rig["sched"])
        else:
            self.ctx.ensure_sampler(T)
            net._bind()
            self.batch = SceneBatch(guides)
            self.batch._bind()
        _capi.check(self.lib.edmp_sampler_set_condition(self.ctx.h, 1))
        self.s = _capi.as_pd(np.ascontiguousarray(rig["starts"][:S] if S > 1 else rig["starts"][0], dtype=np.float64))
        self.g = _capi.as_pd(np.ascontiguousarray(rig["goals"][:S] if S > 1 else rig["goals"][0], dtype=np.float64))
        self.seeds = tuple(SEEDS3[:S] if seeds is None else seeds)
        self.err = lambda: _capi.load().edmp_last_error().decode()

    def out(self):
        o = self.ctx.empty((self.rows, 7, 50), torch.float64)
        o.fill_(float("nan"))
        return o

    def _p(self, o):
        return self.ptr(o) if o is not None else None

    def rng_segment(self, t_hi, t_lo, init, o, seeds=None):
        seeds = self.seeds if seeds is None else seeds
        if self.S == 1:
            return self.lib.edmp_denoise_guided_rng_segment_dev(self.ctx.h, seeds[0], self.B, self.s, self.g, 1, t_hi, t_lo, init, 1, self._p(o))
        arr = (C.c_uint64 * self.S)(*seeds)
        return self.lib.edmp_denoise_scenes_rng_segment_dev(self.ctx.h, arr, self.S, self.B, self.s, self.g, 1, t_hi, t_lo, init, 1, self._p(o))

    def rng_run(self, t_stop, o):
        if self.S == 1:
            return self.lib.edmp_denoise_guided_rng_dev(self.ctx.h, self.seeds[0], self.B, self.s, self.g, 1, t_stop, 1, self._p(o))
        arr = (C.c_uint64 * self.S)(*self.seeds)
        return self.lib.edmp_denoise_scenes_rng_dev(self.ctx.h, arr, self.S, self.B, self.s, self.g, 1, t_stop, 1, self._p(o))

    def explicit_segment(self, noise, t_hi, t_lo, init, o):
        if self.S == 1:
            return self.lib.edmp_denoise_guided_segment_dev(self.ctx.h, self.ptr(noise), self.B, self.s, self.g, 1, t_hi, t_lo, init, 1, self._p(o))
        return self.lib.edmp_denoise_scenes_segment_dev(self.ctx.h, self.ptr(noise), self.S, self.B, self.s, self.g, 1, t_hi, t_lo, init, 1, self._p(o))

    def host(self, o):
        return self.ctx.to_host(o)


@pytest.mark.parametrize("n_scenes", [1, 3])
def test_segments_equal_the_unsegmented_run(net, dif, rig, n_scenes):
    a = _Abi(net, dif, rig, n_scenes)
    two, one, whole = a.out(), a.out(), a.out()
    assert a.rng_segment(T, T - 3, 1, None) == 0, a.err()
    # (a continuing segment reads the recorded seeds, not its argument)
    assert a.rng_segment(T - 3, T - 6, 0, two, seeds=tuple(s ^ 0xFFFF for s in a.seeds)) == 0, a.err()
    assert a.rng_segment(T, T - 6, 1, one) == 0, a.err()
    assert a.rng_run(T - 6, whole) == 0, a.err()
    two, one, whole = a.host(two), a.host(one), a.host(whole)
    assert np.isfinite(whole).all()
    assert np.array_equal(two, one), _differs(two, one)
    assert np.array_equal(one, whole), _differs(one, whole)


@pytest.mark.parametrize("n_scenes", [1, 3])
def test_a_segment_of_the_other_source_is_refused(net, dif, rig, n_scenes):
    a = _Abi(net, dif, rig, n_scenes)
    noise = a.ctx.empty((4, a.rows, 7, 50), torch.float64)
    noise.zero_()
    o = a.out()

    def refused(rc, *words):
        msg = a.err()
        assert rc == ERR_STATE and all(w in msg for w in words), (rc, msg)
        assert torch.isnan(o).all().item()  # nothing was launched

    both = ("device noise source", "explicit noise stream")
    # a device-noise init, then an explicit-noise continuation: refused, and the run goes on under its own source
    assert a.rng_segment(T, T - 3, 1, None) == 0, a.err()
    refused(a.explicit_segment(noise, T - 3, T - 6, 0, o), *both)
    kept = a.out()
    assert a.rng_segment(T - 3, T - 6, 0, kept) == 0, a.err()
    # the reverse
    assert a.explicit_segment(noise, T, T - 3, 1, None) == 0, a.err()
    refused(a.rng_segment(T - 3, T - 6, 0, o), *both)
    # a continuation after a completed run
    whole = a.out()
    assert a.rng_run(T - 6, whole) == 0, a.err()
    refused(a.rng_segment(T - 6, T - 9, 0, o), "no run in progress", "device noise source")
    # the refusals left nothing behind: the continued run and a fresh one are the unsegmented run
    again = a.out()
    assert a.rng_run(T - 6, again) == 0, a.err()
    kept, whole, again = a.host(kept), a.host(whole), a.host(again)
    assert np.isfinite(whole).all() and np.array_equal(kept, whole) and np.array_equal(again, whole)


def test_a_smaller_batch_after_a_larger_one_reads_no_stale_seed(net, dif, rig):
    from edmp_amd.diffusion import DeviceNoise
    from edmp_amd.guide import SceneBatch

    B = rig["B"]
    dif.denoise_guided_scenes(net, SceneBatch(rig["guides"]), 50, 7, rig["starts"], rig["goals"], noise=DeviceNoise(seeds=(11, 12, 13)), t_stop=T - 6)
    seeds = (21, 22)
    two = SceneBatch(rig["guides"][1:])
    got = dif.denoise_guided_scenes(net, two, 50, 7, rig["starts"][1:], rig["goals"][1:], noise=DeviceNoise(seeds=seeds), t_stop=T - 6)
    for k, s in enumerate((1, 2)):
        ref = dif.denoise_guided(net, rig["guides"][s], 50, 7, rig["sched"], batch_size=B, start=rig["starts"][s], goal=rig["goals"][s], noise="device",
                                 seed=seeds[k], t_stop=T - 6)
        assert np.array_equal(got[k], ref), (k, _differs(got[k], ref))


def test_graph_replay_carries_this_call_s_seeds(net, dif, rig):
    from edmp_amd.diffusion import DeviceNoise
    from edmp_amd.guide import SceneBatch

    batch = SceneBatch(rig["guides"])
    sa, sb = DeviceNoise(seeds=(1, 2, 3)), DeviceNoise(seeds=(4, 2, 2**40))

    def run(noise):
        return dif.denoise_guided_scenes(net, batch, 50, 7, rig["starts"], rig["goals"], noise=noise, t_stop=T - 6)

    eager_a, eager_b = run(sa), run(sb)
    assert not np.array_equal(eager_a[0], eager_b[0]) and not np.array_equal(eager_a[2], eager_b[2])
    assert np.array_equal(eager_a[1], eager_b[1])  # (scene 1 keeps its seed: its neighbours' seeds do not reach it)
    dif.set_graph_replay(True)
    try:
        first, second, third = run(sa), run(sb), run(sa)
    finally:
        dif.set_graph_replay(False)
    assert np.array_equal(first, eager_a), _differs(first, eager_a)
    assert np.array_equal(second, eager_b), _differs(second, eager_b)
    assert np.array_equal(third, eager_a), _differs(third, eager_a)
