"""Host side of the device noise source in every run form (no GPU): the DeviceNoise value class and its argument checks, which must
refuse before the GPU is touched; the driver's scene_seed rule; the new entry points in the binding and the header; and the string form
noise="device", which keeps its meaning and its refusals."""
import os
import re

import numpy as np
import pytest

from tests.util import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_device_noise_validates_on_construction():
    from edmp_amd.diffusion import DeviceNoise

    one = DeviceNoise(np.int64(7))
    assert one.single and one.seeds == (7,) and isinstance(one.seeds[0], int)
    assert DeviceNoise(0).seeds == (0,) and DeviceNoise(2**64 - 1).seeds == (2**64 - 1,)
    many = DeviceNoise(seeds=[2**64 - 1, 0, 0])  # equal seeds are allowed
    assert not many.single and many.seeds == (2**64 - 1, 0, 0)
    assert not DeviceNoise(seeds=[5]).single  # one scene is still a scene batch
    for bad in (-1, 2**64, -2**63):
        with pytest.raises(ValueError, match="2\\^64"):
            DeviceNoise(bad)
        with pytest.raises(ValueError, match="2\\^64"):
            DeviceNoise(seeds=[0, bad])
    for bad in (1.0, "1", True, None, [1]):
        with pytest.raises(TypeError, match="integer"):
            DeviceNoise(seeds=[bad])
    with pytest.raises(ValueError):
        DeviceNoise()
    with pytest.raises(ValueError):
        DeviceNoise(1, seeds=[1])
    with pytest.raises(ValueError):
        DeviceNoise(seeds=[])


@pytest.mark.parametrize("warm", [False, True], ids=["full", "warm"])
@pytest.mark.parametrize("case", ["seeds_to_single", "allreduce", "single_to_batch", "too_few", "too_many"])
def test_device_noise_is_checked_before_the_gpu_is_touched(case, warm):
    from edmp_amd.diffusion import DeviceNoise, WarmStart

    S, B = 3, 4
    dif, batch, model = _fakes(S, B)
    z7 = np.zeros(7)
    kw = {}
    with pytest.raises(ValueError):
        if case in ("seeds_to_single", "allreduce"):
            if warm:
                kw["warm_start"] = WarmStart(np.zeros((7, 50)), 32)
            if case == "allreduce":
                kw["allreduce"] = lambda t: None
            noise = DeviceNoise(seeds=[1]) if case == "seeds_to_single" else DeviceNoise(1)
            dif.denoise_guided(model, None, 50, 7, None, batch_size=B, start=z7, goal=z7, noise=noise, **kw)
        else:
            if warm:
                kw["warm_start"] = WarmStart(np.zeros((S, 7, 50)), 32)
            noise = {"single_to_batch": DeviceNoise(1), "too_few": DeviceNoise(seeds=[1, 2]), "too_many": DeviceNoise(seeds=[1, 2, 3, 4])}[case]
            dif.denoise_guided_scenes(model, batch, 50, 7, np.zeros((S, 7)), np.zeros((S, 7)), noise=noise, **kw)


def test_the_string_form_keeps_its_refusals():
    from edmp_amd import _capi
    from edmp_amd.diffusion import WarmStart

    S, B = 3, 4
    dif, batch, model = _fakes(S, B)
    z7 = np.zeros(7)
    with pytest.raises(ValueError, match="no segment form"):
        dif.denoise_guided(model, None, 50, 7, None, batch_size=B, start=z7, goal=z7, noise="device", warm_start=WarmStart(np.zeros((7, 50)), 32))
    with pytest.raises(ValueError, match="no segment form"):
        dif.denoise_guided_scenes(model, batch, 50, 7, np.zeros((S, 7)), np.zeros((S, 7)), noise="device", warm_start=WarmStart(np.zeros((S, 7, 50)), 32))
    with pytest.raises(_capi.EdmpError, match="no scene batch"):
        dif.denoise_guided_scenes(model, batch, 50, 7, np.zeros((S, 7)), np.zeros((S, 7)), noise="device")


def test_scene_seed():
    from infer_serial import scene_seed

    step = 0x9E3779B97F4A7C15
    for seed in (0, 11, 2**64 - 1):
        assert scene_seed(seed, 0) == seed
    assert scene_seed(11, 1) == 11 + step and scene_seed(11, 2) == (11 + 2 * step) % 2**64
    assert scene_seed(2**64 - 1, 1) == step - 1  # the wrap at 2^64
    assert scene_seed(0, 2) == (2 * step) % 2**64 < step
    assert all(0 <= scene_seed(2**63, i) < 2**64 and isinstance(scene_seed(2**63, i), int) for i in range(64))
    # a function of (SEED, i) alone: however the scenes are grouped or dealt to ranks, scene i gets the same seed
    flat = [scene_seed(11, i) for i in range(7)]
    grouped = [scene_seed(11, i) for g0 in range(0, 7, 3) for i in range(g0, min(g0 + 3, 7))]
    dealt = {i: scene_seed(11, i) for rank in range(2) for i in range(7) if i % 2 == rank}
    assert grouped == flat and [dealt[i] for i in range(7)] == flat and len(set(flat)) == 7


def test_driver_refuses_a_seed_outside_uint64():
    import infer_serial

    cfg = os.path.join(ROOT, "configs", "cfg_c1_plumbing.yaml")
    for bad in (-1, 2**64):
        with pytest.raises(ValueError, match="2\\^64"):
            infer_serial.run(cfg, verbose=False, device_noise=bad)


def test_rng_symbols_are_declared_bound_and_exported():
    from edmp_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "edmp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(edmp_[a-z0-9_]+)\s*\(", hdr))
    lib = _capi.load()  # dlopen works without a GPU
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, nargs in (("edmp_denoise_guided_rng_segment_dev", 11), ("edmp_denoise_scenes_rng_dev", 10), ("edmp_denoise_scenes_rng_segment_dev", 12),
                        ("edmp_sampler_seed_rng_dev", 11), ("edmp_sampler_seed_scenes_rng_dev", 12)):
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name) and f"`{name}`" in table, name
        assert len(_capi.SIGNATURES[name][1]) == nargs, name
    # no context: refused before anything touches a device
    assert lib.edmp_denoise_guided_rng_segment_dev(None, 1, 1, None, None, 0, T, T - 1, 1, 1, None) == -1
    assert b"edmp_denoise_guided_rng_segment_dev" in lib.edmp_last_error()
    assert lib.edmp_sampler_seed_rng_dev(None, None, 1, 1, 1, 1, None, None, 0, 32, None) == -1 and b"edmp_sampler_seed_rng_dev" in lib.edmp_last_error()
    assert lib.edmp_denoise_scenes_rng_dev(None, None, 1, 1, None, None, 0, 0, 1, None) == -1
    assert lib.edmp_denoise_scenes_rng_segment_dev(None, None, 1, 1, None, None, 0, T, T - 1, 1, 1, None) == -1
    assert lib.edmp_sampler_seed_scenes_rng_dev(None, None, 1, None, 1, 1, 1, None, None, 0, 32, None) == -1
