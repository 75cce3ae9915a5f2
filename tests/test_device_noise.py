"""The device noise source (noise="device": tail.h rng_normal8, Philox4x32-10 + Box-Muller) against an exact NumPy reference
(oracle/device_rng.py), and the four kernels that draw it (rng_normal_kernel, init_state_rng_kernel, head_psample_kernel<*, true, *>,
the LV_UP_FINAL level kernel through TailP::rng) against one another.  Statistics alone would pass a wrong multiplier or Weyl
constant, a swapped counter or key word, sin and cos swapped or channels permuted: every one of those is O(1) off the reference."""
import numpy as np
import pytest

from oracle import device_rng as R
from tests.util import FULL_DIMS, T, cfgs_for

DEV = "cuda:0"

# Random123's known-answer vectors for philox4x32_10 (counter, key, output)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

# error of the kernel's float32 logf / sqrtf / sincospif path, in float32 ulps of max(|z|, 1): 2.07 measured on an MI355X over the whole
# grid of test_device_noise_matches_the_philox_reference.  A wrong constant, counter word or key word, or sin and cos swapped, is ~1e7 off.
MAX_ULPS = 3.0
ULP1 = 2.0**-23


@pytest.mark.parametrize("ctr,key,out", PHILOX_KAT)
def test_philox_reference_reproduces_random123(ctr, key, out):
    got = R.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == out
    # vectorised over the counter: the same words at every position of an array
    arr = R.philox4x32_10(np.array([ctr[0]] * 3, dtype=np.uint64), *ctr[1:], *key)
    assert all((a == w).all() for a, w in zip(arr, out))


def test_device_noise_reference_layout():
    """(B, C, N)[b, c, l] = z8[b N + l][c]; the channels of one element come from two Philox blocks (blk 0: channels 0-3)"""
    z8 = R.rng_normal8(5, 3, 2 * 50)
    z = R.device_noise(5, 3, 2, 7, 50)
    assert z.shape == (2, 7, 50) and z[1, 4, 17] == z8[50 + 17, 4] and z[0, 6, 0] == z8[0, 6]
    u = R.philox4x32_10(50 + 17, 3, 1, 0, 5, 0)
    u1 = (np.float32(int(u[0])) + np.float32(1)) * np.float32(2.3283064365386963e-10)
    u2 = np.float32(int(u[1])) * np.float32(2.3283064365386963e-10)
    assert z[1, 4, 17] == np.sqrt(-2 * np.log(np.float64(u1))) * np.cos(2 * np.pi * np.float64(u2))
    assert R.device_noise(2**64 - 1, 1, 1, 3, 4).shape == (1, 3, 4)


def _ulps(dev, ref):
    return np.abs(dev - ref) / (ULP1 * np.maximum(np.abs(ref), 1.0))


@pytest.mark.gpu
def test_device_noise_matches_the_philox_reference():
    """Diffusion.device_noise (rng_normal_kernel) == the float64 reference to a few float32 ulps, over both key words of the seed,
    counter steps up to the C-ABI's int limit, ragged and large batches, both horizons and 2 / 3 / 7 channels"""
    from edmp_amd.diffusion import Diffusion

    dif = Diffusion(T, DEV)
    worst = 0.0
    for seed in (0, 1, 2**32 + 7, 2**64 - 1):
        for step in (0, 1, 255, 2**31 - 1):
            z8 = R.rng_normal8(seed, step, 1024 * 64)
            for B in (1, 37, 1024):
                for N in (50, 64):
                    for C in (2, 3, 7):
                        ref = np.ascontiguousarray(z8[:B * N, :C].reshape(B, N, C).transpose(0, 2, 1))
                        got = dif.device_noise(seed, step, B, C, N)
                        e = _ulps(got, ref)
                        worst = max(worst, float(e.max()))
                        assert e.max() <= MAX_ULPS, (seed, step, B, N, C, float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
    print(f"\n[device noise] worst error vs the float64 reference: {worst:.2f} float32 ulps of max(|z|, 1)")


def _program_tail(net):
    """which kernel runs the step tail of the device-resident loop: the last op of the layer program decides"""
    net._bind()
    last = [n for n, _, _, _ in net.ctx.prof_ops()][-1]
    return "level" if last.startswith(("level_kernel<2,", "level2_kernel<1,")) else "psample"


@pytest.mark.gpu
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "unguided"])
@pytest.mark.parametrize("program", ["level", "psample"])
def test_device_noise_loop_equals_the_loop_fed_its_stream(program, guided):
    """A whole run (t = 255 .. 1, so the row-0 zeroing of t = 1 takes part, B > 1) with noise="device" equals the same run fed
    device_noise(seed, k) for every k: init_state_rng_kernel and the step tail - inside the LV_UP_FINAL level kernel, or
    head_psample_kernel<*, true, *> (EDMP_NO_LEVEL=1) - draw exactly what rng_normal_kernel draws, in both FINISH branches
    (guided and unguided steps) and with the seed's high key word in use."""
    import os

    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.temporalunet import TemporalUNet

    old = os.environ.get("EDMP_NO_LEVEL")
    if program == "psample":
        os.environ["EDMP_NO_LEVEL"] = "1"
    try:  # the builder reads its switches when the model is built
        net = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, seed=4, max_batch=8)
        assert _program_tail(net) == program
    finally:
        if old is None:
            os.environ.pop("EDMP_NO_LEVEL", None)
        else:
            os.environ["EDMP_NO_LEVEL"] = old
    dif = Diffusion(T, DEV)
    s, g = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    if guided:
        cfgs = cfgs_for([1, 10], 3)
        B, sched = cfgs["total_batch_size"], cfgs["guidance_schedule"]
        guide = IntersectionVolumeGuide(scenes.random_scene(6, 8), DEV, cfgs, B)
    else:
        B, sched, guide = 5, None, None
    seed = 2**32 + 7
    Xd = dif.denoise_guided(net, guide, 50, 7, sched, batch_size=B, start=s, goal=g, noise="device", seed=seed)
    stream = np.stack([dif.device_noise(seed, k, B) for k in range(T + 1)])
    Xs = dif.denoise_guided(net, guide, 50, 7, sched, batch_size=B, start=s, goal=g, noise=stream)
    assert np.isfinite(Xd).all()
    assert np.array_equal(Xd, Xs), (float(np.abs(Xd - Xs).max()), np.argwhere(Xd != Xs)[:5].tolist())
    # the stream itself is the reference's (one step checked here: the full check is test_device_noise_matches_the_philox_reference)
    assert _ulps(stream[T], R.device_noise(seed, T, B, 7, 50)).max() <= MAX_ULPS
