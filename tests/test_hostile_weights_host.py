"""CPU: the hostile weight families of tests/hostile_weights.py reach their regime in EVERY Conv1dBlock of every architecture the
GPU test (tests/test_gpu_hostile_activations.py) runs, the oracle stays usable as a yardstick there, and the regime decides what it
is meant to decide: an oracle with GroupNorm's eps taken away, or with the fast Mish's clamp taken away, computes something else.
Everything here is the float32 / float64 oracle; no device code runs."""
import numpy as np
import pytest
import torch

from tests import hostile_weights as H
from tests.util import rmse


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("arch", H.ARCHS)
def test_every_block_reaches_the_regime_and_the_regime_decides(arch, kind):
    """At B = 5 and the GPU test's t = 255 / 1, from regime_census (the float64 oracle), in every Conv1dBlock:
      offset    the median over (row, group) of |mean| / std >= 20
      flat      in every row a group with var < 1e-7, one inside 1e-6 ... 1e-4, one > 1e-2
      dead      in every row exactly one group with var == 0
      saturate  max Mish input >= 50, min <= -50, at least 1 % of the inputs inside [19, 21]; both Mish calls of the time embedding
                see a value > 20 and a value < -20, and a value > 45 (past the overflow of n (n + 2) at 44.4)
    The float32 and float64 oracles are finite, and torch-float32's own rmse against float64 stays below 1e-4 x the rms of the
    float64 values on eps and on every tap: a condition on the yardstick the GPU test measures the kernels with (there the bar is
    3 x that error), not a gate on any kernel.
    The proofs that the inputs decide: on `flat` the oracle with eps = 0 differs from the oracle with eps = 1e-5 by more than 100 x
    torch-float32's own float64 error, on `dead` it is not finite; on `saturate` the oracle with the unclamped rational Mish
    n (n + 2) / (n (n + 2) + 2) is not finite."""
    sd = H.arch_state_dict(arch, kind)
    x = H.arch_input(arch)[: H.B_HOST]
    for t in H.TS:
        census = H.regime_census(sd, x, t)
        assert len(census["blocks"]) == len(H.conv_blocks(sd))
        for name, blk in census["blocks"].items():
            var, m = blk["var"], blk["mish"]
            assert var.shape == (H.B_HOST, H.GROUPS)
            if kind == "offset":
                assert np.median(blk["ratio"]) >= 20.0, (name, t, float(np.median(blk["ratio"])))
            elif kind == "flat":
                assert (var < 1e-7).any(axis=1).all(), (name, t, var.min(axis=1))
                assert ((var > 1e-6) & (var < 1e-4)).any(axis=1).all(), (name, t, var)
                assert (var > 1e-2).any(axis=1).all(), (name, t, var.max(axis=1))
            elif kind == "dead":
                assert ((var == 0.0).sum(axis=1) == 1).all(), (name, t, (var == 0.0).sum(axis=1))
            else:
                assert m["max"] >= 50.0 and m["min"] <= -50.0 and m["in_19_21"] >= 0.01, (name, t, m)
        if kind == "saturate":
            for call, m in census["time"].items():
                assert m["max"] > 20.0 and m["min"] < -20.0, (call, t, m)
                assert m["max"] > 45.0, (call, t, m)  # where n (n + 2) has left float32: a rational Mish in the time table would show
        y32, tr32 = H.oracle_forward(sd, x, t)
        y64, tr64 = H.oracle_forward(sd, x, t, torch.float64)
        own = {"eps": rmse(y32, y64) / _rms(y64)}
        assert np.isfinite(y32).all() and np.isfinite(y64).all(), (arch, kind, t)
        for k in tr64:
            assert np.isfinite(tr32[k]).all() and np.isfinite(tr64[k]).all(), (arch, kind, t, k)
            own[k] = rmse(tr32[k], tr64[k]) / _rms(tr64[k])
        worst = max(own, key=own.get)
        print(f"\n[{arch}/{kind} t={t}] torch-f32's own rmse against float64 / rms: eps {own['eps']:.2e}, worst {worst} {own[worst]:.2e}")
        assert own[worst] < 1e-4, (arch, kind, t, worst, own[worst])
        if kind in ("flat", "dead"):
            with np.errstate(all="ignore"):
                y0, _ = H.oracle_forward(sd, x, t, gn_eps=0.0)
            if kind == "dead":
                assert not np.isfinite(y0).all(), (arch, t)
            else:
                assert np.isfinite(y0).all() and rmse(y0, y32) > 100.0 * rmse(y32, y64), (arch, t, rmse(y0, y32), rmse(y32, y64))
                print(f"[{arch}/{kind} t={t}] eps = 0 moves the float32 oracle by x{rmse(y0, y32) / rmse(y32, y64):.3g} its own float64 error")
        if kind == "saturate":
            yn, _ = H.oracle_forward(sd, x, t, mish_fn=H.unclamped_rational_mish)
            assert not np.isfinite(yn).all(), (arch, t)


@pytest.mark.parametrize("case", sorted(H.KNOWN_K_LOOP_EXCESS), ids=lambda c: f"{c[0]}-{c[1]}")
def test_known_excess_comes_with_the_epilogues_inputs(case):
    """The claim behind hostile_weights.KNOWN_K_LOOP_EXCESS, on the CPU, B = 5: two float32 evaluations of the oracle, each with ONE of
    the two things a device kernel does differently from torch's CPU arithmetic.
      E1  torch's convolutions, the epilogue in the device's form (two-pass variance, x s + (beta - s mean), clamped rational Mish)
      E2  the k = 5 convolutions with serial K sums (one accumulator, as a matrix-pipe K loop), torch's own GroupNorm and Mish
    E1 stays inside the 3.0 bar of the GPU test on eps and on every tap at both t - the epilogue's form alone does not reach it
    (measured x1.26 at most).  At every listed (tap, t) E2's error is larger than E1's: the larger part of the excess
    arrives with the epilogue's inputs.  (Measured E2: A2 mid x3.01; FULL down4 / down5 / mid x2.08 / x2.52 / x2.59.  One
    serial order on the CPU is not the device's order, so E2 is the size of the effect, not the device's figure: the GPU test holds
    the device to 3.0 x E2's error at these taps.)"""
    from tests.util import f64_error_ratio

    kind, prog = case
    arch = prog.split("/")[0]
    sd, x = H.arch_state_dict(arch, kind), H.arch_input(arch)[: H.B_HOST]
    known = H.KNOWN_K_LOOP_EXCESS[case]
    for t in H.TS:
        y32, tr32 = H.oracle_forward(sd, x, t)
        y64, tr64 = H.oracle_forward(sd, x, t, torch.float64)
        y1, tr1 = H.oracle_forward(sd, x, t, gn_fn=H.device_form_group_norm, mish_fn=H.clamped_rational_mish)
        for k in ["eps"] + list(tr64):
            q1 = f64_error_ratio(*((y1, y32, y64) if k == "eps" else (tr1[k], tr32[k], tr64[k])))
            assert q1 <= 3.0, (case, t, k, q1)
        taps = [k for k, tt in known if tt == t]
        if not taps:
            continue
        _, tr2 = H.oracle_forward(sd, x, t, conv_fn=H.serial_k_conv)
        for k in taps:
            q1, q2 = f64_error_ratio(tr1[k], tr32[k], tr64[k]), f64_error_ratio(tr2[k], tr32[k], tr64[k])
            print(f"\n[{kind} {prog} t={t}] {k}: device-form epilogue x{q1:.2f}, serial K sums x{q2:.2f} torch-f32's own float64 error")
            assert q2 > q1, (case, t, k, q1, q2)


def test_the_families_change_only_what_they_name():
    """Against weights.init_state_dict with the same seed: `offset` changes conv biases only, `flat` and `dead` the k = 5 conv weights
    and biases only, `saturate` the GroupNorm affine parameters of channels c mod 4 != 3 and the two time-embedding weights only -
    and every family changes every Conv1dBlock."""
    from edmp_amd import weights as W
    from tests import plan_record as R

    cin, td, dims, _ = R.archs()["A3"]
    base = W.init_state_dict(H.SEED, cin, td, dims)
    allowed = {"offset": (".block.0.bias",), "flat": (".block.0.weight", ".block.0.bias"), "dead": (".block.0.weight", ".block.0.bias"),
               "saturate": (".block.2.weight", ".block.2.bias", "time_embedding.time_mlp.1.weight", "time_embedding.time_mlp.3.weight")}
    for kind in H.KINDS:
        sd = H.hostile_state_dict(kind, H.SEED, cin, td, dims)
        assert list(sd) == list(base) and all(sd[k].dtype == np.float32 and sd[k].shape == base[k].shape for k in sd)
        changed = [k for k in sd if not np.array_equal(sd[k], base[k])]
        assert all(k.endswith(allowed[kind]) for k in changed), (kind, changed)
        for p in H.conv_blocks(sd):
            assert any(k.startswith(p + ".block.") for k in changed), (kind, p)
        if kind == "saturate":
            for p in H.conv_blocks(sd):
                assert np.array_equal(sd[p + ".block.2.weight"][3::4], base[p + ".block.2.weight"][3::4])
                assert np.array_equal(sd[p + ".block.2.bias"][3::4], base[p + ".block.2.bias"][3::4])
