"""GPU: warm starts - the device loop begun at an intermediate step from a prior plan (edmp_sampler_seed_dev / _scenes_dev,
Diffusion.denoise_guided(..., warm_start=WarmStart(x0, t_start, renoise))).

Every comparison is bit for bit (np.array_equal on the raw arrays): the library against itself - a resumed run against the uninterrupted
one, one noise source against another, a scene batch against its scenes' own runs - or against the NumPy expression of the forward
process, which edmp_q_sample_dev already meets exactly.  Shapes: T = 255, the tiny net, 12 rows of guides [1, 10, 11, 18, 9, 13] x 2
(iv, sv and grad_norm rows), 7 obstacles, noise_for(5, 12).  One runtime.Context(0) per test, closed when the test leaves its `with Rig(...)`; the uninterrupted
runs every test compares with are computed once, on a context of their own."""
import numpy as np
import pytest
import torch

from tests.util import FULL_DIMS, T, TINY_DIMS, cfgs_for, noise_for

pytestmark = pytest.mark.gpu

PB = 12
P_GUIDES = [1, 10, 11, 18, 9, 13]
NO = 7
ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def inp():
    from edmp_amd import scenes
    from edmp_amd import weights as W

    rs = np.random.RandomState(321)
    d = dict(scene=scenes.random_scene(47, NO), cfgs=cfgs_for(P_GUIDES, 2), noise=noise_for(5, PB), sd=W.init_state_dict(5, 7, 32, TINY_DIMS))
    d["start"], d["goal"] = (np.ascontiguousarray(v, dtype=np.float64) for v in scenes.random_start_goal(3))
    d["x0_rows"] = rs.standard_normal((PB, 7, 50))   # one plan per row
    d["x0_one"] = rs.standard_normal((7, 50))        # one plan for the batch
    d["eps"] = rs.standard_normal((PB, 7, 50))
    return d


class Rig:
    """one context with the net, the probe's guide and the T = 255 diffuser"""

    def __init__(self, inp, dims=TINY_DIMS, sd=None, max_batch=64):
        from edmp_amd.diffusion import Diffusion
        from edmp_amd.guide import IntersectionVolumeGuide
        from edmp_amd.runtime import Context
        from edmp_amd.temporalunet import TemporalUNet

        self.inp = inp
        self.ctx = Context(0)
        try:
            self.net = TemporalUNet(None, 7, 32, self.ctx, dims=dims, state_dict=sd if sd is not None else inp["sd"], max_batch=max_batch)
            self.guide = IntersectionVolumeGuide(inp["scene"], self.ctx, inp["cfgs"], PB)
            self.dif = Diffusion(T, self.ctx)
        except BaseException:
            self.ctx.close()
            raise
        self.lib = self.ctx.lib

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()
        return False

    def run(self, guide="own", **kw):
        """Diffusion.denoise_guided on the rig's objects with the probe's pair"""
        i = self.inp
        g = self.guide if guide == "own" else guide
        kw.setdefault("start", i["start"])
        kw.setdefault("goal", i["goal"])
        return self.dif.denoise_guided(self.net, g, 50, 7, i["cfgs"]["guidance_schedule"] if g is not None else None, batch_size=PB, **kw)

    def bind(self, condition=1, guide="own"):
        from edmp_amd import _capi

        g = self.guide if guide == "own" else guide
        self.dif._prepare(self.net, g, PB, None)
        _capi.check(self.lib.edmp_sampler_set_condition(self.ctx.h, condition))

    def dev(self, a):
        return self.ctx.to_dev(np.ascontiguousarray(a, dtype=np.float64), torch.float64)

    def seed(self, x0, eps, t_start, guided=1, x0_rows=None, B=PB, pair=None, want_out=True):
        """(rc, message, seeded state or None) of one edmp_sampler_seed_dev call"""
        from edmp_amd import _capi
        from edmp_amd.runtime import ptr

        s, g = pair if pair is not None else (self.inp["start"], self.inp["goal"])
        x0d, ed = self.dev(x0), (self.dev(eps) if eps is not None else None)
        out = self.ctx.empty((B, 7, 50), torch.float64) if want_out else None
        rows = x0_rows if x0_rows is not None else (1 if np.ndim(x0) == 2 else len(x0))
        rc = self.lib.edmp_sampler_seed_dev(self.ctx.h, ptr(x0d), rows, ptr(ed) if ed is not None else None, B, _capi.as_pd(s), _capi.as_pd(g), guided, t_start,
                                            ptr(out) if out is not None else None)
        msg = _capi.load().edmp_last_error().decode()
        self.ctx.sync()
        return rc, msg, (self.ctx.to_host(out) if rc == 0 and out is not None else None)

    def seg(self, noise_dev, t_hi, t_lo, guided=1, out=None):
        """(rc, message) of one continuing segment; noise_dev[0] is the draw of step t_hi"""
        from edmp_amd import _capi
        from edmp_amd.runtime import ptr

        i = self.inp
        rc = self.lib.edmp_denoise_guided_segment_dev(self.ctx.h, ptr(noise_dev), PB, _capi.as_pd(i["start"]), _capi.as_pd(i["goal"]), guided, t_hi, t_lo, 0, 1,
                                                      ptr(out) if out is not None else None)
        return rc, _capi.load().edmp_last_error().decode()

    def sentinel(self):
        out = self.ctx.empty((PB, 7, 50), torch.float64)
        with torch.cuda.stream(self.ctx.stream):
            out.fill_(float("nan"))
        return out


@pytest.fixture(scope="module")
def ref(inp):
    """the uninterrupted runs on a context without history: guided, unguided, and the states both stand at after step k + 1"""
    with Rig(inp) as rig:
        out = dict(guided=rig.run(noise=inp["noise"]), unguided=rig.run(guide=None, noise=inp["noise"]))
        for k in (254, 37, 6, 1):
            out[f"guided@{k}"] = rig.run(noise=inp["noise"], t_stop=k)
        out["unguided@37"] = rig.run(guide=None, noise=inp["noise"], t_stop=37)
        out["alpha_bar"] = rig.dif.alpha_bar.copy()
    assert not np.array_equal(out["guided"], out["unguided"]) and np.isfinite(out["guided"]).all()
    return out


def _noised(ab, t, x0, eps):
    """q(x_t | x_0) as NumPy evaluates it: what edmp_q_sample_dev returns bit for bit with cumulative = 1"""
    return np.sqrt(ab[t - 1]) * x0 + np.sqrt(1 - ab[t - 1]) * eps


def _pinned(X, start, goal):
    X = np.array(X)
    X[:, :, 0], X[:, :, -1] = start, goal
    return X


# ---- 1. the seeded state -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("condition", [1, 0])
def test_seed_state_is_the_forward_process_with_the_runs_pins(inp, ref, condition):
    ab = ref["alpha_bar"]
    with Rig(inp) as rig:
        rig.bind(condition)
        for t in (1, 7, 128, 255):
            for x0 in (inp["x0_rows"], inp["x0_one"]):
                for eps in (inp["eps"], None):
                    rc, msg, X = rig.seed(x0, eps, t)
                    assert rc == 0, (t, msg)
                    want = np.broadcast_to(x0, (PB, 7, 50)) if eps is None else _noised(ab, t, x0, eps)
                    if condition:
                        want = _pinned(want, inp["start"], inp["goal"])
                    assert want.shape == X.shape and np.array_equal(X, want), (t, np.ndim(x0), eps is None, condition)
        # the pins are the run's pair, not x0's own end columns
        assert not np.array_equal(inp["x0_one"][:, 0], inp["start"])


# ---- 2. a resume equals the uninterrupted run ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [254, 37, 6, 1])
def test_resume_equals_the_uninterrupted_run(inp, ref, k):
    """254: nearly the whole loop; 37: an unguided step comes first; 6: the last guided step; 1: quirk Q3's row-0 step"""
    from edmp_amd.diffusion import WarmStart

    Z = inp["noise"]
    with Rig(inp) as rig:
        Xk = rig.run(noise=Z, t_stop=k)
        assert np.array_equal(Xk, ref[f"guided@{k}"])
        rig.run(noise=Z, t_stop=T - 2)  # (the state and the UNet input the stopped run left behind are replaced: the seed must bring both)
        got = rig.run(noise=Z[1 + T - k:], warm_start=WarmStart(Xk, k, renoise=False))
    assert np.array_equal(got, ref["guided"])


def test_resume_equals_the_uninterrupted_run_unguided(inp, ref):
    from edmp_amd.diffusion import WarmStart

    with Rig(inp) as rig:
        got = rig.run(guide=None, noise=inp["noise"][1 + T - 37:], warm_start=WarmStart(ref["unguided@37"], 37, renoise=False))
        one = rig.dif.denoise(rig.net, 50, 7, start=inp["start"], goal=inp["goal"], batch_size=PB, noise=inp["noise"][1 + T - 37:],
                              warm_start=WarmStart(ref["unguided@37"], 37, renoise=False))
    assert np.array_equal(got, ref["unguided"]) and np.array_equal(one, got)


def test_resume_equals_the_uninterrupted_run_full_size_net(inp):
    """the full-size net ends in the fused final level, whose launch writes the NEXT step's UNet input: the first step of a resumed run
    must find in its place the input the seed kernel wrote"""
    from edmp_amd import weights as W
    from edmp_amd.diffusion import WarmStart

    Z = inp["noise"]
    with Rig(inp, dims=FULL_DIMS, sd=W.init_state_dict(11, 7, 32, FULL_DIMS), max_batch=PB) as rig:
        full = rig.run(noise=Z)
        Xk = rig.run(noise=Z, t_stop=37)
        rig.run(noise=Z, t_stop=T - 2)  # (what the stopped run left in the model's input buffer is replaced)
        got = rig.run(noise=Z[1 + T - 37:], warm_start=WarmStart(Xk, 37, renoise=False))
    assert np.isfinite(full).all() and not np.array_equal(Xk, full) and np.array_equal(got, full)


# ---- 3. re-noising equals its manual composition ---------------------------------------------------------------------------------
def _renoise_case(inp, t_start):
    x0 = inp["x0_one"] if t_start == 32 else inp["x0_rows"]
    return x0, inp["noise"][:1 + t_start]  # [eps][z of t_start] ... [z of 1]


@pytest.mark.parametrize("t_start", [32, 255])
def test_renoise_equals_seed_then_resume(inp, ref, t_start):
    from edmp_amd.diffusion import WarmStart

    x0, Z = _renoise_case(inp, t_start)
    with Rig(inp) as rig:
        rig.bind(1)
        rc, msg, Xs = rig.seed(x0, Z[0], t_start)
        assert rc == 0, msg
        assert np.array_equal(Xs, _pinned(_noised(ref["alpha_bar"], t_start, x0, Z[0]), inp["start"], inp["goal"]))
        manual = rig.run(noise=Z[1:], warm_start=WarmStart(Xs, t_start, renoise=False))
        whole = rig.run(noise=Z, warm_start=WarmStart(x0, t_start, renoise=True))
        stopped = rig.run(noise=Z[:1 + t_start - 5], warm_start=WarmStart(x0, t_start), t_stop=5)
        rest = rig.run(noise=Z[1 + t_start - 5:], warm_start=WarmStart(stopped, 5, renoise=False))
    assert np.isfinite(whole).all() and np.array_equal(manual, whole) and np.array_equal(rest, whole)
    assert not np.array_equal(whole, ref["guided"])


# ---- 4. the noise sources agree ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("renoise", [True, False])
def test_noise_sources_agree(inp, renoise):
    from edmp_amd.diffusion import PinnedNoiseStream, WarmStart

    draws = (1 if renoise else 0) + 32
    np.random.seed(77)
    Z = np.random.standard_normal((draws, PB, 7, 50))
    marker = np.random.standard_normal()
    ws = lambda: WarmStart(inp["x0_rows"], 32, renoise=renoise)  # noqa: E731
    with Rig(inp) as rig:
        got = dict(ndarray=rig.run(noise=Z, warm_start=ws()))
        got["device"] = rig.run(noise=torch.tensor(Z, device=rig.ctx.device), warm_start=ws())
        pin = torch.from_numpy(Z.copy()).pin_memory()
        got["pinned"] = rig.run(noise=pin, warm_start=ws())
        stream = PinnedNoiseStream(pin)
        stream.publish(pin.numel())
        got["stream"] = rig.run(noise=stream, warm_start=ws())
        got["short chunks"] = rig.run(noise=pin, warm_start=ws(), chunk_steps=3)
        np.random.seed(77)
        got["numpy"] = rig.run(warm_start=ws())
        assert np.random.standard_normal() == marker  # exactly `draws` draws of (B, C, N) were taken, in that order
        x0d = torch.tensor(inp["x0_rows"], device=rig.ctx.device)
        dev = rig.run(noise=Z, warm_start=WarmStart(x0d, 32, renoise=renoise), return_device=True)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda
        got["device x0, device result"] = dev.cpu().numpy()
    assert np.isfinite(got["ndarray"]).all()
    for k, v in got.items():
        assert np.array_equal(v, got["ndarray"]), k


# ---- 5. a scene batch ----------------------------------------------------------------------------------------------------------------
def test_scene_batch_equals_its_scenes_own_warm_starts(inp):
    from edmp_amd import scenes
    from edmp_amd.diffusion import WarmStart
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch

    S = 3
    rs = np.random.RandomState(55)
    sg = [scenes.random_start_goal(110 + k) for k in range(S)]
    starts, goals = np.stack([a for a, _ in sg]), np.stack([b for _, b in sg])
    Z = [rs.standard_normal((33, PB, 7, 50)) for _ in range(S)]
    x0s = {"per scene": rs.standard_normal((S, 7, 50)), "per row": rs.standard_normal((S, PB, 7, 50))}
    sched = inp["cfgs"]["guidance_schedule"]
    with Rig(inp) as rig:
        guides = [IntersectionVolumeGuide(scenes.random_scene(100 + k, 4 + 3 * k), rig.ctx, inp["cfgs"], PB) for k in range(S)]
        batch = SceneBatch(guides)
        for tag, x0 in x0s.items():
            own = [rig.run(guide=guides[k], start=starts[k], goal=goals[k], noise=Z[k], warm_start=WarmStart(x0[k], 32)) for k in range(S)]
            assert not np.array_equal(own[0], own[1])
            got = rig.dif.denoise_guided_scenes(rig.net, batch, 50, 7, starts, goals, noise=Z, warm_start=WarmStart(x0, 32))
            assert got.shape == (S, PB, 7, 50)
            for k in range(S):
                assert np.array_equal(got[k], own[k]), (tag, k)
            pins = [torch.from_numpy(z.copy()).pin_memory() for z in Z]
            assert np.array_equal(rig.dif.denoise_guided_scenes(rig.net, batch, 50, 7, starts, goals, noise=pins, warm_start=WarmStart(x0, 32)), got), tag
        # a resume of the batch (no eps draw), its streams drawn from the global NumPy state in scene order; unguided with per-scene pins
        x0 = x0s["per row"]
        np.random.seed(78)
        Zr = [np.random.standard_normal((32, PB, 7, 50)) for _ in range(S)]
        marker = np.random.standard_normal()
        a = rig.dif.denoise_guided_scenes(rig.net, batch, 50, 7, starts, goals, noise=Zr, warm_start=WarmStart(x0, 32, renoise=False))
        np.random.seed(78)
        b = rig.dif.denoise_guided_scenes(rig.net, batch, 50, 7, starts, goals, warm_start=WarmStart(x0, 32, renoise=False))
        assert np.random.standard_normal() == marker and np.array_equal(a, b)
        u = rig.dif.denoise_guided_scenes(rig.net, batch, 50, 7, starts, goals, noise=Z, warm_start=WarmStart(x0, 32), guided=False)
        for k in range(S):
            assert np.array_equal(u[k], rig.run(guide=None, start=starts[k], goal=goals[k], noise=Z[k], warm_start=WarmStart(x0[k], 32))), k


# ---- 6. bookkeeping ----------------------------------------------------------------------------------------------------------------
def test_seeded_run_bookkeeping_and_refusals(inp, ref):
    """a seed call is the init of a run that stands at t_start: the continuing segment must bring that step, the run ends by what ends
    any segmented run, and every refusal launches nothing and leaves no trace in the next full run"""
    from edmp_amd import _capi, scenes
    from edmp_amd.diffusion import WarmStart
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch
    from edmp_amd.runtime import ptr

    x0, Z = inp["x0_one"], inp["noise"]
    with Rig(inp) as rig:
        zd = rig.dev(Z[1:33])  # draws of steps 32 .. 1
        eps = Z[0]

        def full_run_is_clean(what):
            assert np.array_equal(rig.run(noise=Z), ref["guided"]), what
            rig.bind(1)

        rig.bind(1)
        out = rig.sentinel()
        untouched = lambda: torch.isnan(out).all().item()  # noqa: E731
        # the segment must start where the seed stands
        rc, msg, _ = rig.seed(x0, eps, 32)
        assert rc == 0, msg
        rc, msg = rig.seg(zd, 31, 0, out=out)
        assert rc == ERR_STATE and "32" in msg and "31" in msg and untouched(), (rc, msg)
        rc, msg = rig.seg(zd, 32, 0, out=out)
        assert rc == 0, msg
        want32 = rig.ctx.to_host(out)
        assert np.array_equal(want32, rig.run(noise=Z[:33], warm_start=WarmStart(x0, 32)))
        full_run_is_clean("segment at the wrong step")
        # a run seeded unguided cannot be continued guided; unguided it goes on
        out = rig.sentinel()
        rc, msg, _ = rig.seed(x0, eps, 32, guided=0)
        assert rc == 0, msg
        rc, msg = rig.seg(zd, 32, 0, guided=1, out=out)
        assert rc == ERR_STATE and "unguided" in msg and untouched(), (rc, msg)
        rc, msg = rig.seg(zd, 32, 0, guided=0, out=out)
        assert rc == 0 and np.array_equal(rig.ctx.to_host(out), rig.run(guide=None, noise=Z[:33], warm_start=WarmStart(x0, 32))), msg
        full_run_is_clean("guided continuation of an unguided seed")
        # the row-volume call replaces the guide's pair: the run is over
        out = rig.sentinel()
        rc, msg, _ = rig.seed(x0, eps, 32)
        assert rc == 0, msg
        rig.guide.row_swept_volumes(inp["goal"], inp["start"], ref["guided"])
        rc, msg = rig.seg(zd, 32, 0, out=out)
        assert rc == ERR_STATE and "no run in progress" in msg and untouched(), (rc, msg)
        full_run_is_clean("row volumes between seed and segment")
        # arguments out of range: nothing launched (the state output keeps its sentinel), no run left behind
        for t_bad in (0, T + 1):
            sent = rig.sentinel()
            x0d, ed = rig.dev(x0), rig.dev(eps)
            rc = rig.lib.edmp_sampler_seed_dev(rig.ctx.h, ptr(x0d), 1, ptr(ed), PB, _capi.as_pd(inp["start"]), _capi.as_pd(inp["goal"]), 1, t_bad, ptr(sent))
            msg = _capi.load().edmp_last_error().decode()
            rig.ctx.sync()
            assert rc == ERR_ARG and str(t_bad) in msg and torch.isnan(sent).all().item(), (t_bad, rc, msg)
            rc, msg = rig.seg(zd, 32, 0, out=out)
            assert rc == ERR_STATE and untouched(), (t_bad, rc, msg)
            full_run_is_clean(f"t_start = {t_bad}")
        rc, msg, _ = rig.seed(inp["x0_rows"][:5], eps, 32, x0_rows=5)
        assert rc == ERR_ARG and "5" in msg, (rc, msg)
        full_run_is_clean("x0_rows = 5")
        # the Python refusals come before anything is enqueued
        with pytest.raises(ValueError, match="device"):
            rig.run(noise="device", warm_start=WarmStart(x0, 32))
        with pytest.raises(ValueError, match="allreduce"):
            rig.run(noise=Z[:33], warm_start=WarmStart(x0, 32), allreduce=lambda t: None)
        full_run_is_clean("device noise / allreduce with a warm start")
        # the single-scene seed on a bound scene batch, and the scene seed on a single-scene guide
        S = 3
        guides = [IntersectionVolumeGuide(scenes.random_scene(100 + k, 4 + 3 * k), rig.ctx, inp["cfgs"], PB) for k in range(S)]
        batch = SceneBatch(guides)
        batch._bind()
        rc, msg, _ = rig.seed(x0, eps, 32)
        assert rc == ERR_STATE and "scene batch" in msg, (rc, msg)
        full_run_is_clean("single-scene seed on a bound scene batch")
        sent = rig.ctx.empty((S * PB, 7, 50), torch.float64)
        with torch.cuda.stream(rig.ctx.stream):
            sent.fill_(float("nan"))
        x0d, ed = rig.dev(np.stack([x0] * S)), rig.dev(np.concatenate([eps] * S))
        sg = np.ascontiguousarray(np.stack([inp["start"]] * S)), np.ascontiguousarray(np.stack([inp["goal"]] * S))
        rc = rig.lib.edmp_sampler_seed_scenes_dev(rig.ctx.h, ptr(x0d), S, ptr(ed), S, PB, _capi.as_pd(sg[0]), _capi.as_pd(sg[1]), 1, 32, ptr(sent))
        msg = _capi.load().edmp_last_error().decode()
        rig.ctx.sync()
        assert rc == ERR_STATE and "scene" in msg and torch.isnan(sent).all().item(), (rc, msg)
        rc = rig.lib.edmp_sampler_seed_scenes_dev(rig.ctx.h, ptr(x0d), 5, ptr(ed), S, PB, _capi.as_pd(sg[0]), _capi.as_pd(sg[1]), 0, 32, ptr(sent))
        assert rc == ERR_ARG and torch.isnan(sent).all().item(), (rc, _capi.load().edmp_last_error().decode())
        full_run_is_clean("scene seed on a single-scene guide")
        # and the seeded run still works on this context
        assert np.array_equal(rig.run(noise=Z[:33], warm_start=WarmStart(x0, 32)), want32)


# ---- 7. history ----------------------------------------------------------------------------------------------------------------------
def test_warm_start_ignores_the_contexts_history(inp):
    from edmp_amd import scenes
    from edmp_amd.diffusion import WarmStart
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch

    x0, Z = _renoise_case(inp, 32)
    with Rig(inp) as rig:
        first = rig.run(noise=Z, warm_start=WarmStart(x0, 32))
        rs = np.random.RandomState(36)
        s, e = scenes.random_start_goal(51)
        # a full 255-step run at another B
        rig.dif.denoise_guided(rig.net, None, 50, 7, None, batch_size=20, start=s, goal=e, noise=rs.standard_normal((T + 1, 20, 7, 50)))
        # a scene-batch run: other start / goal pairs in the sampler, 36 rows of state
        guides = [IntersectionVolumeGuide(scenes.random_scene(60 + k, no), rig.ctx, inp["cfgs"], PB) for k, no in enumerate((3, 7, 16))]
        sg = [scenes.random_start_goal(40 + k) for k in range(3)]
        rig.dif.denoise_guided_scenes(rig.net, SceneBatch(guides), 50, 7, np.stack([a for a, _ in sg]), np.stack([b for _, b in sg]),
                                      noise=[rs.standard_normal((T + 1, PB, 7, 50)) for _ in range(3)], t_stop=T - 60)
        # condition=False as the last loop call, warm-started itself
        X = rig.run(noise=Z, warm_start=WarmStart(x0, 32), condition=False, start=s, goal=e)
        assert not np.allclose(X[:, :, 0], s)
        again = rig.run(noise=Z, warm_start=WarmStart(x0, 32))
    assert np.isfinite(first).all() and np.array_equal(first, again)
    with Rig(inp) as rig:
        assert np.array_equal(rig.run(noise=Z, warm_start=WarmStart(x0, 32)), first)
