"""GPU: the four copies of the GroupNorm -> Mish epilogue (csrc/bf3.hip, wide.hip, level.hip, gn_mish_kernel of unet.hip) and the
three Mish functions of csrc/common.h on the hostile weight families of tests/hostile_weights.py: group means far above the group's
deviation (`offset`), group variances around and below GroupNorm's eps (`flat`), a variance of exactly zero (`dead`), Mish inputs
beyond +-50 and around the softplus threshold 20, in the UNet and in the time table (`saturate`).  tests/test_hostile_weights_host.py
proves on the CPU that every Conv1dBlock of every architecture used here is in the regime and that the regime decides the result.

Programs: every row of tests/instance_programs.py: PROGRAMS (every listed wide_, bf3_, level_ and level2_ instance), A2 on the
generic kernels and A10 (gn_mish_kernel<2>, <4>, <8>, the generic conv and rcb_ kernels), TINY.  Per family and program one forward
at B = 37 and t = 255 / 1; eps and every activation tap against the float64 oracle.  The gates are the project's own: finite wherever
float64 is finite; rmse against float64 <= 3 x torch-float32's own (tests.util.f64_error_ratio, the bar of
test_architecture_vs_oracle); a B = 5 forward bit-identical to the first five rows; and for FULL the adoption bar of
test_bf16x3_split_layers_are_at_least_as_accurate_as_the_fp32_mfma_layers between the default build and EDMP_BF16X3=0.  The fixed
float32 gates of the suite (rmse 2e-5 s, max 2e-4 s) are not applied: on `offset` torch-float32 itself is up to 30 x less accurate
than on random weights (recorded below), so they would measure against the wrong yardstick.
The measured figures go to profiles/hostile_activations.json, written once every record of a run of the WHOLE module is in: a partial
run (-k, -x, one test id) writes nothing."""
import json
import os

import numpy as np
import pytest
import torch

from tests import hostile_weights as H
from tests import instance_programs as P
from tests import plan_record as R
from tests.taps import missing_tap_explained, tap_ids, tap_key
from tests.test_gpu_archs import DEV, _env, _op_names
from tests.util import f64_error_ratio, maxabs, rmse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGS = tuple((r.arch, r.env) for r in P.PROGRAMS) + (("A2", {"EDMP_NO_FUSED": "1"}), ("A10", {}), ("TINY", {}))
NATIVE = ("FULL", {"EDMP_BF16X3": "0"})  # the fp32-MFMA build the bf16x3 layers were adopted against
ADOPTION_TAPS = ("down2", "down3", "down4", "up1", "up2")
assert {a for a, _ in PROGS} == set(H.ARCHS)

# Cases above the bar whose excess is not the epilogue's: tests/hostile_weights.py: KNOWN_K_LOOP_EXCESS, keyed by (tap, t).  Such a
# case is held strictly - exactly the listed (tap, t) stand above 3.0, every other tap and t is held to 3.0 as everywhere - and has a
# ceiling: on the listed taps the device stays within 3.0 x the float64 error of a float32 oracle whose k = 5 convolutions sum their
# products serially (hostile_weights.serial_k_conv), i.e. the same bar against a float32 yardstick that sums as a K loop does.
_REFS, _RUNS, _NAMES, _SERIAL = {}, {}, {}, {}


def _serial_k_refs(arch, kind, t):
    """(eps, taps) of the float32 oracle with serial K sums on the first B_HOST rows (a row's forward does not depend on the others)"""
    if (arch, kind, t) not in _SERIAL:
        _SERIAL[(arch, kind, t)] = H.oracle_forward(H.arch_state_dict(arch, kind), H.arch_input(arch)[: H.B_HOST], t, conv_fn=H.serial_k_conv)
    return _SERIAL[(arch, kind, t)]
RECORD = {"f64_ratio": {}, "adoption": {}}


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))


def _refs(arch, kind):
    """t -> (eps32, taps32, eps64, taps64) of the oracle at B = 37, computed once per (architecture, family) and never written to"""
    if (arch, kind) not in _REFS:
        sd, x = H.arch_state_dict(arch, kind), H.arch_input(arch)
        out = {}
        for t in H.TS:
            y32, tr32 = H.oracle_forward(sd, x, t)
            y64, tr64 = H.oracle_forward(sd, x, t, torch.float64)
            out[t] = (y32, tr32, y64, tr64)
        _REFS[(arch, kind)] = out
    return _REFS[(arch, kind)]


def _run(kind, prog):
    """one construction, and per t one forward at B = 37 with every tap read and one at B = 5: {"names", t: (eps, taps, eps at B = 5)}"""
    key = (kind, P.program_id(prog))
    if key not in _RUNS:
        from edmp_amd import _capi
        from edmp_amd.temporalunet import TemporalUNet

        arch, env = prog
        cin, td, dims, n = R.archs()[arch]
        with _env(**env):  # the builder reads its switches when a model is built
            net = TemporalUNet(None, cin, td, DEV, dims=dims, state_dict=H.arch_state_dict(arch, kind), max_batch=H.B_GPU, horizon=n)
        out = {"names": _op_names(net)}
        _NAMES[P.program_id(prog)] = out["names"]
        x = torch.from_numpy(H.arch_input(arch))
        for t in H.TS:
            tt = torch.tensor([float(t)])
            eps = net(x, tt).cpu().numpy()
            taps = {}
            for w in tap_ids(len(dims)):
                try:
                    taps[tap_key(w)] = net.activation(w, H.B_GPU).cpu().numpy()
                except _capi.EdmpError:
                    assert missing_tap_explained(w, len(dims), out["names"]), f"tap {w} missing from a program without a merge that explains it"
            out[t] = (eps, taps, net(x[: H.B_HOST], tt).cpu().numpy())
        _RUNS[key] = out
    return _RUNS[key]


def _record(section, key, value):
    """profiles/hostile_activations.json, written once every figure of a whole run of this module is in"""
    RECORD[section][key] = value
    if len(RECORD["f64_ratio"]) == len(H.KINDS) * len(PROGS) and len(RECORD["adoption"]) == len(H.KINDS):
        per_family = {k: {p: v for (kk, p), v in RECORD["f64_ratio"].items() if kk == k} for k in H.KINDS}
        rec = dict(test="tests/test_gpu_hostile_activations.py", device=torch.cuda.get_device_name(0),
                   constants=dict(OFFSET=H.OFFSET, SAT_GAIN=H.SAT_GAIN, SAT_BIAS=H.SAT_BIAS, SAT_EDGE_GAIN=H.SAT_EDGE_GAIN,
                                  TIME_SCALE_1=H.TIME_SCALE_1, TIME_SCALE_3=H.TIME_SCALE_3, seed=H.SEED, B=H.B_GPU, t=list(H.TS)),
                   f64_ratio=dict(measure="rmse against the float64 oracle over torch-float32's own (floor 1e-7 x rms), worst of t = 255 / 1, on eps and "
                                          "on the worst activation tap (gate 3.0); torch_f32_own: torch-float32's rmse against float64 / rms of the "
                                          "float64 values, same worst-of (the yardstick's own error, host-gated below 1e-4)", per_family=per_family),
                   adoption=dict(measure="FULL, default build (bf16x3 layers) over EDMP_BF16X3=0 (fp32 MFMA): ratio of the rmse / of the max error "
                                         "against float64, worst of eps and the taps down2 ... up2 and of t = 255 / 1 (gates 1.25 / 1.5)",
                                 per_family=RECORD["adoption"]))
        with open(os.path.join(ROOT, "profiles", "hostile_activations.json"), "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


@pytest.mark.parametrize("prog", PROGS, ids=P.program_id)
@pytest.mark.parametrize("kind", H.KINDS)
def test_epilogues_on_hostile_statistics(kind, prog):
    """One program on one family (the module's docstring): finite, eps and every tap within 3 x torch-float32's own float64 error,
    the B = 5 forward bit-identical to the first five rows of B = 37.  Measured over the 44 cases: eps x0.79 ... x1.83, worst tap
    x0.83 ... x2.95, and the two cases of hostile_weights.KNOWN_K_LOOP_EXCESS (x3.16 on mid at t = 1; x3.63 / x3.36 / x3.14 on
    down4 / down5 / mid at t = 1).  Those two are reported as expected failures only while exactly the listed (tap, t) stand above
    3.0, nothing else of the case fails, and the listed taps stay within 3.0 x the serial-K float32 oracle's own float64 error."""
    arch, _ = prog
    run, refs = _run(kind, prog), _refs(arch, kind)
    if PROGS.index(prog) < len(P.PROGRAMS):  # a row of the instance table: the instances it answers for are in the bound program
        row = P.PROGRAMS[PROGS.index(prog)]
        assert not [n for n in P.there_for(row) if n not in run["names"]], (P.there_for(row), run["names"])
    fails, over_bar = [], {}
    worst, own = {"eps": 0.0, "tap": 0.0, "which": None}, {"eps": 0.0, "tap": 0.0, "which": None}
    for t in H.TS:
        eps, taps, eps5 = run[t]
        y32, tr32, y64, tr64 = refs[t]
        assert eps.shape == y64.shape and set(taps) <= set(tr64)
        if not np.array_equal(eps5, eps[: H.B_HOST]):
            fails.append(f"t={t}: the B = {H.B_HOST} forward differs from the same rows inside B = {H.B_GPU} (max {maxabs(eps5, eps[: H.B_HOST]):.3e})")
        for name, a, r32, r64 in [("eps", eps, y32, y64)] + [(k, taps[k], tr32[k], tr64[k]) for k in taps]:
            if a.shape != r64.shape:
                fails.append(f"t={t} {name}: shape {a.shape} != {r64.shape}")
                continue
            bad = np.isfinite(r64) & ~np.isfinite(a)
            if bad.any():
                fails.append(f"t={t} {name}: {int(bad.sum())} of {a.size} values not finite where float64 is")
                continue
            q, o = f64_error_ratio(a, r32, r64), rmse(r32, r64) / _rms(r64)
            print(f"[{kind} {P.program_id(prog)} t={t}] {name}: x{q:.2f} torch-f32's own float64 error ({o:.2e} of rms)")
            slot = "eps" if name == "eps" else "tap"
            if q > worst[slot]:
                worst[slot] = q
                if slot == "tap":
                    worst["which"] = f"{name}@t={t}"
            if o > own[slot]:
                own[slot] = o
                if slot == "tap":
                    own["which"] = f"{name}@t={t}"
            if not q <= 3.0:
                over_bar[(name, t)] = f"t={t} {name} vs f64: x{q:.2f} torch-f32's error"
    known = H.KNOWN_K_LOOP_EXCESS.get((kind, P.program_id(prog)))
    ceiling = {}
    for name, t in known or ():  # the same bar against the float32 oracle that sums its K products serially, on the first B_HOST rows
        ys, ts = _serial_k_refs(arch, kind, t)
        a = (run[t][0] if name == "eps" else run[t][1][name])[: H.B_HOST]
        r64 = (refs[t][2] if name == "eps" else refs[t][3][name])[: H.B_HOST]
        ceiling[f"{name}@t={t}"] = q = f64_error_ratio(a, ys if name == "eps" else ts[name], r64)
        print(f"[{kind} {P.program_id(prog)} t={t}] {name}: x{q:.2f} the serial-K float32 oracle's own float64 error (rows 0 .. {H.B_HOST - 1})")
        if not q <= 3.0:
            fails.append(f"t={t} {name} vs f64: x{q:.2f} the serial-K float32 oracle's error")
    _record("f64_ratio", (kind, P.program_id(prog)),
            dict(eps=round(worst["eps"], 3), worst_tap=round(worst["tap"], 3), tap=worst["which"],
                 torch_f32_own=dict(eps=float(f"{own['eps']:.3g}"), worst_tap=float(f"{own['tap']:.3g}"), tap=own["which"]),
                 passed=not fails and not over_bar, known_k_loop_excess=sorted(f"{n}@t={t}" for n, t in known) if known else None,
                 vs_serial_k_oracle={k: round(v, 3) for k, v in ceiling.items()} if known else None))
    if known:
        assert not fails, "beyond the known K-loop excess:\n" + "\n".join(fails)
        assert set(over_bar) == set(known), (f"the (tap, t) above the bar are not the ones of KNOWN_K_LOOP_EXCESS {sorted(known)}:\n"
                                             + "\n".join(over_bar.values()))
        pytest.xfail("K-loop excess, not the epilogue's (KNOWN_K_LOOP_EXCESS): " + "; ".join(over_bar.values()))
    assert not fails and not over_bar, "\n".join(fails + list(over_bar.values()))


@pytest.mark.parametrize("kind", H.KINDS)
def test_bf16x3_adoption_bar_on_hostile_statistics(kind):
    """FULL with the default switches (the bf16x3 layers) against FULL with EDMP_BF16X3=0 (fp32 MFMA), on eps and on the taps down2 ...
    up2: the split build's rmse against float64 <= 1.25 x the native build's, its max error <= 1.5 x - the adoption bar of
    test_bf16x3_split_layers_are_at_least_as_accurate_as_the_fp32_mfma_layers, on the new families."""
    split, native, refs = _run(kind, ("FULL", {})), _run(kind, NATIVE), _refs("FULL", kind)
    assert any(n.startswith("bf3_") for n in split["names"]) and not any(n.startswith("bf3_") for n in native["names"])
    fails, worst = [], {"rmse": 0.0, "max": 0.0}
    for t in H.TS:
        _, _, y64, tr64 = refs[t]
        rows = [("eps", native[t][0], split[t][0], y64)] + [(k, native[t][1][k], split[t][1][k], tr64[k]) for k in ADOPTION_TAPS]
        for name, n_, s_, r_ in rows:
            assert np.isfinite(n_).all() and np.isfinite(s_).all(), (kind, t, name)
            en, es, mn, ms = rmse(n_, r_), rmse(s_, r_), maxabs(n_, r_), maxabs(s_, r_)
            print(f"[bf16x3/{kind} t={t}] {name}: vs f64 rmse native {en:.3e} split {es:.3e} (x{es / en:.2f}); max native {mn:.3e} split {ms:.3e} (x{ms / mn:.2f})")
            worst["rmse"], worst["max"] = max(worst["rmse"], es / en), max(worst["max"], ms / mn)
            if not (es <= 1.25 * en and ms <= 1.5 * mn):
                fails.append(f"t={t} {name}: rmse x{es / en:.2f} (bar 1.25), max x{ms / mn:.2f} (bar 1.5)")
    _record("adoption", kind, dict(rmse=round(worst["rmse"], 3), max=round(worst["max"], 3), passed=not fails))
    assert not fails, "\n".join(fails)


def test_the_programs_launch_every_epilogue_copy():
    """Read back from the bound programs: between them they launch the Conv1dBlock kernels of bf3.hip and wide.hip (kind 0, and the
    Karatsuba kinds 3 / 4 of wide.hip), the one- and two-level kernels of level.hip, and gn_mish_kernel<2>, <4> and <8>."""
    for prog in PROGS:
        if P.program_id(prog) not in _NAMES:
            _run("dead", prog)
    every = {n for prog in PROGS for n in P.launched(_NAMES[P.program_id(prog)])}
    for prefix in ("bf3_conv_kernel<0,", "wide_conv_kernel<0,", "wide_conv_kernel<3,", "wide_conv_kernel<4,", "level_kernel<0,", "level_kernel<1,",
                   "level_kernel<2,", "level2_kernel<", "gn_mish_kernel<2>", "gn_mish_kernel<4>", "gn_mish_kernel<8>"):
        assert any(n.startswith(prefix) for n in every), (prefix, sorted(every))
    assert not [n for n in P.listed_instances() if n not in every]
