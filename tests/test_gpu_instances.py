"""GPU: every program of tests/instance_programs.py: PROGRAMS runs, and is held to the oracle; a scene batch equals its serial runs in
every level form and in every position-tile family; a row's forward does not depend on where in the batch it sits.

tests/test_instance_coverage_host.py proves on the CPU that PROGRAMS launches every instance csrc/kernel_instances.h lists.  Here each
row is bound and its names are read back (the instances the row answers for are in the bound program); the rows no other test sweeps
go through tests/test_gpu_archs.py: _sweep unchanged (eps and every activation tap at B = 130 / 37 / 1 and t = 255 / 37 / 1 against the
float32 oracle and a float64 evaluation); the programs whose last op is a four-sample level kernel run the fused step tail at batches
whose last workgroup holds 1, 2 and 3 rows.  No tolerance is introduced here: every gate is one of tests/test_gpu_archs.py or
array_equal.  The measured figures go to profiles/instance_coverage.json."""
import json
import os

import numpy as np
import pytest
import torch

from tests import instance_programs as P
from tests.test_gpu_archs import BS, DEV, _arch, _env, _net, _op_names, _sd, _sweep, _teacher_forced
from tests.util import T, cfgs_for, rmse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEPT_HERE = [r for r in P.PROGRAMS if r.swept_by is None]
K6 = 6  # reverse steps of the loop tests (three of them guided): a full 255-step run adds time and nothing else

LEVEL4 = {"EDMP_LEVEL_MERGE": "0", "EDMP_LEVEL_SB": "4444"}
LEVEL2 = {"EDMP_LEVEL_MERGE": "0", "EDMP_LEVEL_SB": "2222"}
DIRECT = {"EDMP_NO_KARATSUBA": "1", "EDMP_BF16X3": "0"}

# program family -> (architecture, switches, modulus): rows of equal content are bit-equal among batch positions congruent modulo
# `modulus` (1: at every position).  The level kernels sum a row's GroupNorm statistics in the order of its slot in the SB-row
# workgroup, so their programs hold the claim modulo SB; every other family has to hold it everywhere.
FAMILIES = {
    "bf3": ("A2", {"EDMP_NO_LEVEL": "1"}, 1),
    "bf3+karatsuba_l2": ("FULL", {"EDMP_NO_LEVEL": "1"}, 1),
    "wide_karatsuba_l4": ("A2", {"EDMP_BF16X3": "0", "EDMP_NO_LEVEL": "1"}, 1),
    "wide_direct": ("A2", dict(DIRECT, EDMP_NO_LEVEL="1"), 1),
    "wide_direct_l2": ("FULL", {"EDMP_NO_KARATSUBA": "1", "EDMP_NO_LEVEL": "1"}, 1),
    "wide_ms32": ("FULL", {"EDMP_BF16X3": "0", "EDMP_MS16": "0", "EDMP_NO_LEVEL": "1"}, 1),
    "wide_ms16": ("FULL", {"EDMP_BF16X3": "0", "EDMP_MS16": "0x1f", "EDMP_NO_LEVEL": "1"}, 1),
    "generic": ("A2", {"EDMP_NO_FUSED": "1"}, 1),
    "level_sb2": ("A2", LEVEL2, 2),
    "level_sb4": ("A2", LEVEL4, 4),
    "level2_sb2": ("A2", {}, 2),
}
RECORD = {"f64_ratio": {}, "position": {}}


def _record(kind, key, value):
    """profiles/instance_coverage.json, written once every figure of a whole run of this module is in"""
    RECORD[kind][key] = value
    if len(RECORD["f64_ratio"]) == len(SWEPT_HERE) and len(RECORD["position"]) == len(FAMILIES):
        rec = dict(test="tests/test_gpu_instances.py", device=torch.cuda.get_device_name(0),
                   f64_ratio=dict(measure="worst rmse against the float64 oracle over torch-float32's own, B = 130, t = 255 / 37 / 1 (gate 3.0): "
                                          "test_program_sweep", per_program=RECORD["f64_ratio"]),
                   position=dict(measure="130 rows cycling three contents, t = 37 and t = 1: max |difference| in eps / in any tap between rows of equal "
                                         "content at positions congruent modulo `modulus` (asserted 0) and at any two positions: "
                                         "test_a_rows_forward_does_not_depend_on_its_position", per_family=RECORD["position"]))
        with open(os.path.join(ROOT, "profiles", "instance_coverage.json"), "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


def _full_net(env, max_batch):
    from edmp_amd.temporalunet import TemporalUNet
    from tests.util import FULL_DIMS

    with _env(**env):
        return TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, seed=4, max_batch=max_batch)


def _build(arch, env, max_batch):
    return _full_net(env, max_batch) if arch == "FULL" else _net(arch, env=env, max_batch=max_batch)


# ---------------------------------------------------------------------------------------------------------------- 1. names
@pytest.mark.parametrize("row", P.PROGRAMS, ids=P.program_id)
def test_bound_program_launches_what_the_row_is_there_for(row):
    """the bound model's program is the described one (so the CPU coverage test speaks about what runs here) and holds every
    instance the row answers for"""
    net = _build(row.arch, row.env, 4)
    names = _op_names(net)
    assert P.launched(names) == P.described(row)
    want = P.there_for(row)
    assert want and not [n for n in want if n not in P.launched(names)], (want, names)
    y = net(torch.zeros(3, 7, 50), torch.tensor([5.0])).cpu().numpy()  # (and it launches: one forward at a ragged batch)
    assert y.shape == (3, 7, 50) and np.isfinite(y).all()


# ---------------------------------------------------------------------------------------------------------------- 2. sweep, step tail
@pytest.mark.parametrize("row", SWEPT_HERE, ids=P.program_id)
def test_program_sweep(row):
    """tests/test_gpu_archs.py: _sweep on a program no other test sweeps: eps and every tap against the float32 oracle (rmse <= 2e-5 s,
    max <= 2e-4 s; taps <= 5e-4 max(1, max|ref| / 8)) and the float64 evaluation (<= 3 x torch-float32's own error), sub-batches
    bit-identical to the same rows of B = 130"""
    net = _net(row.arch, env=row.env)
    names = _op_names(net)
    assert not [n for n in P.there_for(row) if n not in names]
    worst_eps, worst_tap, fails = _sweep(row.arch, net, P.program_id(row))
    _record("f64_ratio", P.program_id(row), dict(eps=round(worst_eps, 3), taps=round(worst_tap, 3)))
    assert not fails, "\n".join(fails)


def _loop_rig(aid, env, B, guides):
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.guide_cfg import split_rows

    net = _net(aid, env=env, max_batch=B)
    cfgs = cfgs_for(guides, 0, rows_per_guide=split_rows(B, len(guides)))
    guide = IntersectionVolumeGuide(scenes.random_scene(5, 12), DEV, cfgs, B)
    return net, guide, Diffusion(T, DEV), cfgs


def _short_stream(rs, B, draws=K6 + 1):
    """a (T + 1, B, 7, 50) stream whose first `draws` draws are normal; the loop tests stop before the others are read"""
    z = np.zeros((T + 1, B, 7, 50))
    z[:draws] = rs.standard_normal((draws, B, 7, 50))
    return z


@pytest.mark.parametrize("B", (37, 6, 7, 5))
def test_four_sample_step_tail_equals_the_stepwise_api(B):
    """test_device_loop_equals_the_stepwise_api_at_full_size on A3 with level_kernel<2, 32, 25, 4, 128> as the last launch: the tail of
    a reverse step inside that launch (final 1x1 conv, posterior, conditioning, next input, the Philox branch) against the stepwise API,
    bit for bit after six steps, three of them guided, and noise="device" against the run fed the materialised stream.  B = 37, 6, 7:
    the last four-sample workgroup holds 1, 2, 3 rows.  B = 5: unguided (FINISH on every step), the short workgroup holds one row."""
    from edmp_amd import scenes

    guided = B != 5
    net, guide, dif, cfgs = _loop_rig("A3", LEVEL4, B, [1, 10, 11])
    assert _op_names(net)[-1] == "level_kernel<2, 32, 25, 4, 128>"
    g, sched = (guide, cfgs["guidance_schedule"]) if guided else (None, None)
    s, gl = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    noise = _short_stream(np.random.RandomState(80 + B), B)
    X_loop = dif.denoise_guided(net, g, 50, 7, sched, batch_size=B, start=s, goal=gl, noise=noise, t_stop=T - K6)
    assert np.isfinite(X_loop).all()
    assert np.array_equal(X_loop[:, :, 0], np.broadcast_to(s, (B, 7))) and np.array_equal(X_loop[:, :, -1], np.broadcast_to(gl, (B, 7)))
    if guided:
        X = noise[0].copy()
        X[:, :, 0], X[:, :, -1] = s, gl
        for k, t in enumerate(range(T, T - K6, -1)):
            X = dif.denoise_step(net, guide, X, noise[1 + k], t, s, gl, sched)["x_out"]
        assert np.array_equal(X_loop, X), (float(np.abs(X_loop - X).max()), int((X_loop != X).sum()), np.argwhere(X_loop != X)[:5].tolist())
    else:
        # the unguided loop has no stepwise twin (the stepwise API guides the even steps): it is held to the oracle's unguided loop,
        # at the gate of test_free_running_unguided_with_other_channel_counts
        from oracle import edmp_oracle as O

        om, (b, a, ab) = O.UNetOracle(_sd("A3"), 32), O.schedule(T)
        Xo = np.array(noise[0])
        Xo[:, :, 0], Xo[:, :, -1] = s, gl
        for k, t in enumerate(range(T, T - K6, -1)):
            eps = om(torch.tensor(Xo, dtype=torch.float32), torch.tensor([float(t)])).numpy()
            Xo = O.p_sample_using_posterior(Xo, t, eps, noise[1 + k], b, a, ab)
            Xo[:, :, 0], Xo[:, :, -1] = s, gl
        print(f"\n[A3 SB = 4 unguided B={B}] {K6} steps: rmse vs oracle {rmse(X_loop, Xo):.3e}")
        assert rmse(X_loop, Xo) <= 1e-4, rmse(X_loop, Xo)
    Xd = dif.denoise_guided(net, g, 50, 7, sched, batch_size=B, start=s, goal=gl, noise="device", seed=77, t_stop=T - K6)
    stream = np.zeros((T + 1, B, 7, 50))
    for k in range(K6 + 1):
        stream[k] = dif.device_noise(77, k, B)
    Xs = dif.denoise_guided(net, g, 50, 7, sched, batch_size=B, start=s, goal=gl, noise=stream, t_stop=T - K6)
    assert np.array_equal(Xd, Xs), (float(np.abs(Xd - Xs).max()), np.argwhere(Xd != Xs)[:5].tolist())
    assert not np.array_equal(Xd, X_loop)


def test_four_sample_step_tail_against_the_float64_posterior():
    """one teacher-forced guided step (t = 254) and one unguided step (t = 253) of the SB = 4 program of A3 against oracle.denoise_step
    at the gates of tests/test_gpu_archs.py: _teacher_forced; X_t comes from the device loop, i.e. through the fused four-sample tail"""
    from oracle import edmp_oracle as O

    with _env(**LEVEL4):  # (_teacher_forced builds its own model: the builder reads the switches then)
        net, _, _, _, _ = _teacher_forced(O, "A3", 37, [1, 10, 11], (254, 253), seed=11)
    assert _op_names(net)[-1] == "level_kernel<2, 32, 25, 4, 128>"


# ---------------------------------------------------------------------------------------------------------------- 3. scene batches
def _scene_rig(rows, S=3):
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.guide_cfg import split_rows

    cfgs = cfgs_for([1, 10], 0, rows_per_guide=split_rows(rows, 2))
    assert cfgs["total_batch_size"] == rows
    guides = [IntersectionVolumeGuide(scenes.random_scene(6 + k, n), DEV, cfgs, rows) for k, n in zip(range(S), (4, 7, 10))]
    starts = np.stack([scenes.DEFAULT_START + 0.01 * k for k in range(S)])
    goals = np.stack([scenes.DEFAULT_GOAL - 0.01 * k for k in range(S)])
    return cfgs, guides, starts, goals


def _scene_batch_equals_serial(net, dif, rows, tag):
    """three scenes of `rows` rows, six reverse steps: guided under explicit noise and unguided under the device source, every scene
    array_equal to its serial run (test_unguided_scene_batch_equals_its_serial_device_runs)"""
    from edmp_amd.diffusion import DeviceNoise
    from edmp_amd.guide import SceneBatch

    S = 3
    cfgs, guides, starts, goals = _scene_rig(rows, S)
    batch = SceneBatch(guides)
    rs = np.random.RandomState(500 + rows)
    noises = [_short_stream(rs, rows) for _ in range(S)]
    got = dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals, noise=noises, t_stop=T - K6)
    assert got.shape == (S, rows, 7, 50) and np.isfinite(got).all()
    bad = []
    for s, g in enumerate(guides):
        ref = dif.denoise_guided(net, g, 50, 7, cfgs["guidance_schedule"], batch_size=rows, start=starts[s], goal=goals[s], noise=noises[s], t_stop=T - K6)
        if not np.array_equal(got[s], ref):
            bad.append(f"{tag} guided, {rows} rows per scene, scene {s}: max |batch - serial| {float(np.abs(got[s] - ref).max()):.3e}, rows {sorted(set(np.argwhere(got[s] != ref)[:, 0].tolist()))}")
    assert not np.array_equal(got[0], got[1])
    seeds = (5, 2**63, 2**64 - 1)
    free = dif.denoise_guided_scenes(net, batch, 50, 7, starts, goals, noise=DeviceNoise(seeds=seeds), guided=False, t_stop=T - K6)
    for s in range(S):
        ref = dif.denoise_guided(net, None, 50, 7, None, batch_size=rows, start=starts[s], goal=goals[s], noise="device", seed=seeds[s], t_stop=T - K6)
        if not np.array_equal(free[s], ref):
            bad.append(f"{tag} unguided, {rows} rows per scene, scene {s}: max |batch - serial| {float(np.abs(free[s] - ref).max()):.3e}, rows {sorted(set(np.argwhere(free[s] != ref)[:, 0].tolist()))}")
    return bad


@pytest.mark.parametrize("aid,env", [("A2", LEVEL4), ("A3", LEVEL4), ("A2", LEVEL2)], ids=["A2/SB=4", "A3/SB=4", "A2/SB=2"])
def test_scene_batch_equals_serial_runs_in_every_level_form(aid, env):
    """the unmerged level_kernel launcher with four and with two samples per workgroup: 3, 5, 6 and 7 rows per scene give a scene only
    a short workgroup, or a full one followed by a short one of 1, 2 or 3 rows (level.hip: level_body deals workgroups scene by scene)"""
    from edmp_amd.diffusion import Diffusion

    net = _net(aid, env=env, max_batch=3 * 7)
    names = _op_names(net)
    sb = env["EDMP_LEVEL_SB"][0]
    assert any(n.startswith("level_kernel<") for n in names) and not any(n.startswith("level2_kernel<") for n in names)
    assert all(n.split(", ")[3] == sb for n in names if n.startswith("level_kernel<")), names
    dif = Diffusion(T, DEV)
    bad = []
    for rows in (3, 5, 6, 7):
        bad += _scene_batch_equals_serial(net, dif, rows, f"{aid}/SB={sb}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("env", [{"EDMP_BF16X3": "0"}, DIRECT, {"EDMP_NO_FUSED": "1"}], ids=["BF16X3=0", "NO_KARATSUBA,BF16X3=0", "NO_FUSED"])
def test_scene_batch_equals_serial_runs_in_the_position_tile_families(env):
    """17 and 33 rows per scene, three scenes: scenes begin at slots 17, 2 (and 1, 2) of the 16- and 32-sample tiles of wide.hip and
    of the generic kernels' 64- / 128-sample tiles, and straddle workgroups"""
    from edmp_amd.diffusion import Diffusion

    net = _net("A2", env=env, max_batch=3 * 33)
    names = _op_names(net)
    assert not any(n.startswith("bf3_") for n in names)
    if "EDMP_NO_FUSED" in env:
        assert not any(n.startswith(("wide_", "level")) for n in names)
    if env is DIRECT:
        assert "wide_conv_kernel<0, 32, 64, 64, 4, true>" in names and "wide_conv_kernel<0, 32, 32, 32, 4, false>" in names
    dif = Diffusion(T, DEV)
    bad = []
    for rows in (17, 33):
        bad += _scene_batch_equals_serial(net, dif, rows, P.program_id(("A2", env)))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------- 4. position
def _taps(net, n_levels, B):
    from edmp_amd import _capi

    out = {}
    for w in list(range(n_levels)) + [100] + [200 + j for j in range(n_levels - 1)]:
        try:
            out[w] = net.activation(w, B).cpu().numpy()
        except _capi.EdmpError:  # a tap the program keeps on chip (tests/test_gpu_archs.py: _missing_tap_explained)
            continue
    return out


def _position_spread(a, modulus, period=3):
    """a: (B, ...) outputs of a batch whose row p holds content p mod `period`.  Max |difference| between rows of equal content at
    positions congruent modulo `modulus`, and between rows of equal content at any positions"""
    B = a.shape[0]
    a = a.reshape(B, -1).astype(np.float64)
    same_slot = anywhere = 0.0
    for c in range(period):
        rows = np.arange(c, B, period)
        anywhere = max(anywhere, float((a[rows].max(axis=0) - a[rows].min(axis=0)).max()))
        for m in range(modulus):
            grp = rows[rows % modulus == m]
            assert len(grp) >= 2
            same_slot = max(same_slot, float((a[grp].max(axis=0) - a[grp].min(axis=0)).max()))
    return same_slot, anywhere


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_rows_forward_does_not_depend_on_its_position(family):
    """130 rows cycling three distinct rows (row p holds content p mod 3), one forward at t = 37 and at t = 1: rows of equal content are
    bit-equal, in eps and in every tap the program has, at every position - in programs with level kernels among positions congruent
    modulo SB, which is what DESIGN section 7 states and what dealing workgroups scene by scene relies on.  A prefix keeps its rows'
    positions, so the prefix checks of the sweeps cannot see a sum whose order depends on a row's slot in its tile; this does."""
    arch, env, modulus = FAMILIES[family]
    B = max(BS)
    net = _build(arch, env, B)
    names = _op_names(net)
    has_level = any(n.startswith("level") for n in names)
    assert has_level == (modulus > 1), names
    n_levels = 6 if arch == "FULL" else len(_arch(arch)[0])
    three = torch.tensor(np.random.RandomState(41).standard_normal((3, 7, 50)) * 1.5, dtype=torch.float32)
    x = three[torch.arange(B) % 3].contiguous()
    worst = dict(eps_same_slot=0.0, eps_anywhere=0.0, tap_same_slot=0.0, tap_anywhere=0.0)
    bad = []
    for t in (37, 1):
        eps = net(x, torch.tensor([float(t)])).cpu().numpy()
        assert np.isfinite(eps).all() and not np.array_equal(eps[0], eps[1])
        for what, a in [("eps", eps)] + [(f"tap {w}", v) for w, v in _taps(net, n_levels, B).items()]:
            same, anyw = _position_spread(a, modulus)
            k = "eps" if what == "eps" else "tap"
            worst[k + "_same_slot"], worst[k + "_anywhere"] = max(worst[k + "_same_slot"], same), max(worst[k + "_anywhere"], anyw)
            if same != 0.0:
                bad.append(f"{family} t={t} {what}: rows of equal content differ by {same:.3e} at positions congruent mod {modulus}")
    print(f"\n[{family}] {arch} {env}: max difference between rows of equal content: {worst}")
    _record("position", family, dict(program=P.program_id((arch, env)), modulus=modulus, **worst))
    assert not bad, "\n".join(bad)
