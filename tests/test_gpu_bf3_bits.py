"""GPU: the bodies of the bf16x3 kernels (csrc/bf3.hip) compute, bit for bit, what they computed at the commit recorded in
tests/golden/bf3_parent_bits.npz (scripts/record_bf3_parent_bits.py), and - independently of that file - what the oracle computes.

The forwards are those of tests/bf3_bits_inputs.py: B = 33, t = 37, default program, on the full architecture (all 16 listed bf16x3
instances, K loops of 2 to 32 chunks) and two three-level ones whose L = 13 instance gets 32 and 96 input channels (K loops of one and of
three chunks).  A reordering of the K loop that changes any accumulator's MFMA sequence, or of the epilogue that changes a GroupNorm
sum, changes bits here.  No tolerance is introduced: array_equal against the fixture, the gates of tests/test_gpu_archs.py: _sweep
against the float32 oracle and its float64 evaluation, array_equal between the device loop and the stepwise API."""
import os

import numpy as np
import pytest
import torch

from tests import bf3_bits_inputs as I
from tests.test_gpu_archs import DEV, _missing_tap_explained, _tap_key
from tests.util import T, cfgs_for, maxabs, rmse
from tests.util import f64_error_ratio as _ratio

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf3_parent_bits.npz")
_RUNS = {}


def _run(name):
    """(op names, eps, taps) of the forward on this tree's library, once per module"""
    if name not in _RUNS:
        net, eps, taps = I.forward(name, DEV)
        net._bind()
        _RUNS[name] = ([n for n, _, _, _ in net.ctx.prof_ops()], eps, taps)
    return _RUNS[name]


@pytest.mark.parametrize("name", tuple(I.ARCHS))
def test_forward_equals_the_parent_commits_bits(name):
    """eps whole, every tap by SHA-256 and by rows 0, 15, 16, 31, 32 whole, against what the recorded parent commit's library gave"""
    g = np.load(GOLDEN, allow_pickle=False)
    assert (int(g["B"]), int(g["t"]), tuple(int(r) for r in g["rows"])) == (I.B, I.T_STEP, I.ROWS)
    ops, eps, taps = _run(name)
    assert ops == [str(s) for s in g[f"{name}_ops"]], "the program changed: re-record the fixture from the parent of the change under test"
    missing = [n for n in (I.BF3_FULL if name == "full" else I.BF3_SMALL) if n not in ops]
    assert not missing, missing
    assert sorted(taps) == g[f"{name}_taps"].tolist()
    bad = []
    ref = g[f"{name}_eps"]
    if not np.array_equal(eps, ref):
        bad.append(f"eps: {int((eps != ref).sum())} of {eps.size} elements differ, max {maxabs(eps, ref):.3e}, first rows {sorted(set(np.argwhere(eps != ref)[:, 0].tolist()))[:6]}")
    for w, a in sorted(taps.items()):
        rows = g[f"{name}_tap{w}_rows"]
        if I.digest(a) != str(g[f"{name}_tap{w}_sha256"]):
            sub = a[list(I.ROWS)]
            bad.append(f"tap {_tap_key(w)}: SHA-256 differs; on rows {I.ROWS}: {int((sub != rows).sum())} of {sub.size} elements differ, max {maxabs(sub, rows):.3e}")
    assert not bad, f"[{name}] against parent commit {str(g['parent_commit'])}:\n" + "\n".join(bad)


_ORACLE = {}


def _oracle(name):
    if name not in _ORACLE:
        from oracle import edmp_oracle as O

        sd32 = {k: torch.from_numpy(v) for k, v in I.state_dict(name).items()}
        sd64 = {k: v.double() for k, v in sd32.items()}
        x = torch.from_numpy(I.x_input(name))
        tr32, tr64 = {}, {}
        with torch.no_grad():
            y32 = O.unet_forward(sd32, x, torch.tensor([float(I.T_STEP)]), I.TIME_DIM, trace=tr32).numpy()
            y64 = O.unet_forward(sd64, x.double(), torch.tensor([float(I.T_STEP)], dtype=torch.float64), I.TIME_DIM, trace=tr64).numpy()
        _ORACLE[name] = (y32, {k: v.numpy() for k, v in tr32.items()}, y64, {k: v.numpy() for k, v in tr64.items()})
    return _ORACLE[name]


@pytest.mark.parametrize("name", tuple(I.ARCHS))
def test_forward_meets_the_oracle_gates(name):
    """the same forward at the gates of tests/test_gpu_archs.py: _sweep: eps against the float32 oracle rmse <= 2e-5 s, max <= 2e-4 s
    (s = max(1, rms)), every tap max <= 5e-4 max(1, max|ref| / 8); eps and taps against float64 <= 3 x torch-float32's own rmse"""
    dims, _ = I.ARCHS[name]
    ops, eps, taps = _run(name)
    y32, tr32, y64, tr64 = _oracle(name)
    fails = []
    s = max(1.0, float(np.sqrt(np.mean(y32 ** 2))))
    q = _ratio(eps, y32, y64)
    print(f"\n[{name}] eps vs f32 oracle: rmse {rmse(eps, y32):.3e} max {maxabs(eps, y32):.3e} (scale {s:.3g}); vs f64: x{q:.2f} torch-f32's error")
    if not (rmse(eps, y32) <= 2e-5 * s and maxabs(eps, y32) <= 2e-4 * s):
        fails.append(f"eps vs f32 oracle: rmse {rmse(eps, y32):.3e} max {maxabs(eps, y32):.3e} (scale {s:.3g})")
    if q > 3.0:
        fails.append(f"eps vs f64: x{q:.2f} torch-f32's error")
    for w in I.taps_of(dims):
        if w not in taps:
            if not _missing_tap_explained(w, len(dims), ops):
                fails.append(f"tap {w} missing from a program without a merge that explains it")
            continue
        k = _tap_key(w)
        a, ra32, ra64 = taps[w], tr32[k], tr64[k]
        if a.shape != ra32.shape:
            fails.append(f"tap {k}: shape {a.shape} != {ra32.shape}")
            continue
        lim = 5e-4 * max(1.0, float(np.abs(ra32).max()) / 8)
        q = _ratio(a, ra32, ra64)
        print(f"[{name}] tap {k}: max {maxabs(a, ra32):.3e} (limit {lim:.3e}); vs f64: x{q:.2f}")
        if maxabs(a, ra32) > lim:
            fails.append(f"tap {k}: max {maxabs(a, ra32):.3e} > {lim:.3e}")
        if q > 3.0:
            fails.append(f"tap {k} vs f64: x{q:.2f} torch-f32's error")
    assert not fails, f"[{name}]\n" + "\n".join(fails)


def test_two_step_device_loop_equals_the_stepwise_api():
    """the full architecture at B = 33: the device-resident loop over t = 255 (unguided) and t = 254 (guided) against two stepwise
    calls, bit for bit, as tests/test_gpu_instances.py: test_four_sample_step_tail_equals_the_stepwise_api does for its program"""
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.guide_cfg import split_rows
    from edmp_amd.temporalunet import TemporalUNet

    B, steps = I.B, 2
    dims, _ = I.ARCHS["full"]
    net = TemporalUNet(None, I.INPUT_DIM, I.TIME_DIM, DEV, dims=dims, state_dict=I.state_dict("full"), max_batch=B, horizon=I.HORIZON)
    cfgs = cfgs_for([1, 10, 11], 0, rows_per_guide=split_rows(B, 3))
    guide = IntersectionVolumeGuide(scenes.random_scene(5, 12), DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    sched = cfgs["guidance_schedule"]
    s, gl = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    noise = np.zeros((T + 1, B, 7, 50))
    noise[:steps + 1] = np.random.RandomState(133).standard_normal((steps + 1, B, 7, 50))
    X_loop = dif.denoise_guided(net, guide, 50, 7, sched, batch_size=B, start=s, goal=gl, noise=noise, t_stop=T - steps)
    assert np.isfinite(X_loop).all()
    X = noise[0].copy()
    X[:, :, 0], X[:, :, -1] = s, gl
    grads = []
    for k, t in enumerate(range(T, T - steps, -1)):
        st = dif.denoise_step(net, guide, X, noise[1 + k], t, s, gl, sched)
        grads.append(st["grad"] is not None)
        X = st["x_out"]
    assert sorted(grads) == [False, True], grads  # one guided and one unguided step
    assert np.array_equal(X_loop, X), (float(np.abs(X_loop - X).max()), int((X_loop != X).sum()), np.argwhere(X_loop != X)[:5].tolist())
