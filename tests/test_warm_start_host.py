"""Host side of warm starts (no GPU): the WarmStart value class, the segment plan of a warm-started run, chunk_plan left as it was,
the two seed entry points in the binding and the header, and the argument checks of the two loop methods, which must refuse a warm
start that does not fit before they touch the GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests.util import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_warm_start_validates_on_construction():
    from edmp_amd.diffusion import WarmStart

    for shape in ((7, 50), (12, 7, 50), (3, 12, 7, 50)):
        w = WarmStart(np.zeros(shape, dtype=np.float32), 32)
        assert w.x0.dtype == np.float64 and w.x0.shape == shape and w.x0.flags["C_CONTIGUOUS"]
        assert w.t_start == 32 and w.renoise and w.lead == 1
    w = WarmStart(np.arange(350).reshape(7, 50), np.int64(7), renoise=False)  # integers convert exactly
    assert w.x0.dtype == np.float64 and isinstance(w.t_start, int) and w.t_start == 7 and w.lead == 0
    assert WarmStart([[0.0, 1.0], [2.0, 3.0]], 1).x0.shape == (2, 2)
    t = torch.zeros((12, 7, 50), dtype=torch.float32)
    assert WarmStart(t, 5).x0 is t  # tensors (host or device) are kept and converted by the call that uses them
    for bad in (np.zeros(50), np.zeros((2, 3, 12, 7, 50)), np.zeros((0, 7, 50)), np.float64(1.0), torch.zeros(50)):
        with pytest.raises(ValueError, match="shape"):
            WarmStart(bad, 32)
    for bad in (np.zeros((7, 50), dtype=np.complex128), np.array([["a"] * 50] * 7), np.zeros((7, 50), dtype=bool), np.full((7, 50), None, dtype=object),
                torch.zeros((7, 50), dtype=torch.bool), torch.zeros((7, 50), dtype=torch.complex64)):
        with pytest.raises(TypeError, match="real numbers"):
            WarmStart(bad, 32)
    for bad in (32.0, "32", None, True, np.float64(3), [3]):
        with pytest.raises(TypeError, match="t_start"):
            WarmStart(np.zeros((7, 50)), bad)


GRID = [(ts, stop, lead, cs) for ts in (1, 2, 3, 16, 17, 32, 37, 128, 255) for stop in sorted({0, ts // 2, ts - 1}) for lead in (0, 1) for cs in (1, 5, 16)]


@pytest.mark.parametrize("t_start,t_stop,lead,chunk_steps", GRID)
def test_warm_plan_is_contiguous_in_steps_and_draws(t_start, t_stop, lead, chunk_steps):
    from edmp_amd.diffusion import chunk_plan, warm_plan

    plan = warm_plan(t_start, t_stop, lead, chunk_steps)
    assert plan and plan[0].t_hi == t_start and plan[-1].t_lo == t_stop
    assert [s.init for s in plan] == [True] + [False] * (len(plan) - 1)
    offset = 0
    for k, s in enumerate(plan):
        assert s.t_hi > s.t_lo and s.t_hi - s.t_lo <= chunk_steps
        assert k == 0 or s.t_hi == plan[k - 1].t_lo          # steps: contiguous, descending
        assert s.offset == offset                             # draws: contiguous
        assert s.draws == s.t_hi - s.t_lo + (lead if k == 0 else 0)
        offset += s.draws
    assert offset == lead + t_start - t_stop
    # the same cuts as a full run's plan from that step; with the lead draw it IS that plan
    base = chunk_plan(t_start, t_stop, chunk_steps)
    assert [(s.t_hi, s.t_lo) for s in plan] == [(s.t_hi, s.t_lo) for s in base]
    if lead:
        assert plan == base


def test_warm_plan_refuses_another_lead():
    from edmp_amd.diffusion import warm_plan

    with pytest.raises(ValueError):
        warm_plan(32, 0, 2)


def test_chunk_plan_is_what_it_was():
    """the feeder of infer_serial.py and the three noise paths work in units of this plan: literal lists, written down before the change"""
    from edmp_amd.diffusion import Segment, chunk_plan

    want0 = [(255, 254, True, 2, 0), (254, 252, False, 2, 2), (252, 248, False, 4, 4), (248, 240, False, 8, 8), (240, 224, False, 16, 16),
             (224, 208, False, 16, 32), (208, 192, False, 16, 48), (192, 176, False, 16, 64), (176, 160, False, 16, 80), (160, 144, False, 16, 96),
             (144, 128, False, 16, 112), (128, 112, False, 16, 128), (112, 96, False, 16, 144), (96, 80, False, 16, 160), (80, 64, False, 16, 176),
             (64, 48, False, 16, 192), (48, 32, False, 16, 208), (32, 16, False, 16, 224), (16, 0, False, 16, 240)]
    assert chunk_plan(255, 0) == [Segment(*w) for w in want0]
    assert chunk_plan(255) == chunk_plan(255, 0, 16)
    want200 = [(255, 254, True, 2, 0), (254, 252, False, 2, 2), (252, 248, False, 4, 4), (248, 240, False, 8, 8), (240, 224, False, 16, 16),
               (224, 208, False, 16, 32), (208, 200, False, 8, 48)]
    assert chunk_plan(255, 200) == [Segment(*w) for w in want200]


def test_seed_symbols_are_declared_bound_and_exported():
    from edmp_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "edmp_hip.h")).read()
    assert "eagerly" in hdr  # the header says that a warm-started run is never replayed from a hipGraph
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(edmp_[a-z0-9_]+)\s*\(", hdr))
    lib = _capi.load()  # dlopen works without a GPU
    for name, nargs in (("edmp_sampler_seed_dev", 10), ("edmp_sampler_seed_scenes_dev", 11)):
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
        assert len(_capi.SIGNATURES[name][1]) == nargs, name
    # no context: refused before anything touches a device
    assert lib.edmp_sampler_seed_dev(None, None, 1, None, 1, None, None, 0, 32, None) == -1 and b"edmp_sampler_seed_dev" in lib.edmp_last_error()
    assert lib.edmp_sampler_seed_scenes_dev(None, None, 1, None, 1, 1, None, None, 0, 32, None) == -1


class _NoGpu:
    """a context stand-in: any use of it means the call went past its argument checks"""

    def __getattr__(self, name):
        raise AssertionError(f"argument checks let the call reach the context ({name})")


def _fakes(S=3, B=4):
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import SceneBatch

    ctx = _NoGpu()
    dif = object.__new__(Diffusion)
    dif.__dict__.update(ctx=ctx, T=T, variance_thresh=0.02)
    batch = object.__new__(SceneBatch)
    batch.__dict__.update(ctx=ctx, n_scenes=S, batch_size=B)

    class Model:
        pass

    m = Model()
    m.__dict__.update(ctx=ctx, horizon=50, input_dim=7, max_batch=S * B)
    return dif, batch, m


CASES = ["not_a_warm_start", "device_noise", "t_start_0", "t_start_256", "t_stop_equal", "t_stop_above", "x0_rows", "x0_len", "noise_steps", "noise_rows",
         "noise_full_length"]


@pytest.mark.parametrize("case,scenes", [(c, sc) for sc in (False, True) for c in CASES] + [("allreduce", False)])  # (the scenes method has no allreduce)
def test_warm_start_is_checked_before_the_gpu_is_touched(case, scenes):
    from edmp_amd.diffusion import WarmStart

    dif, batch, model = _fakes()
    S, B = 3, 4
    x0 = np.zeros((S, 7, 50) if scenes else (7, 50))
    ws, kw = WarmStart(x0, 32), {}
    one = lambda steps, rows=B: np.zeros((steps, rows, 7, 50))  # noqa: E731
    noise = one(33)
    if case == "not_a_warm_start":
        ws = x0
    elif case == "device_noise":
        noise = "device"
    elif case == "t_start_0":
        ws, noise = WarmStart(x0, 0), one(1)
    elif case == "t_start_256":
        ws, noise = WarmStart(x0, T + 1), one(T + 2)
    elif case == "t_stop_equal":
        kw["t_stop"] = 32
    elif case == "t_stop_above":
        kw["t_stop"] = 40
    elif case == "x0_rows":
        ws = WarmStart(np.zeros((S, B + 1, 7, 50) if scenes else (B + 1, 7, 50)), 32)
    elif case == "x0_len":
        ws = WarmStart(np.zeros((S, 7, 48) if scenes else (7, 48)), 32)
    elif case == "noise_steps":
        noise = one(32)  # renoise: the eps draw is missing
    elif case == "noise_rows":
        noise = one(33, B + 1)
    elif case == "noise_full_length":
        noise = one(T + 1)
    elif case == "allreduce":
        kw["allreduce"] = lambda t: None
    with pytest.raises(ValueError):
        if scenes:
            dif.denoise_guided_scenes(model, batch, 50, 7, np.zeros((S, 7)), np.zeros((S, 7)), noise=noise if isinstance(noise, str) else [noise] * S,
                                      warm_start=ws, **kw)
        else:
            dif.denoise_guided(model, None, 50, 7, None, batch_size=B, start=np.zeros(7), goal=np.zeros(7), noise=noise, warm_start=ws, **kw)
