"""GPU: the whole-batch metrics (edmp_metrics_rows_dev, csrc/metrics.hip) and the trust-region pick (edmp_select_row_dev) - SURVEY.md
§8f row 3 at batch size.  Yardsticks: the reference's recorded outputs (tests/golden/g13_metrics.npz) and the single-trajectory host
functions of edmp_amd/evaluation.py, which G13 pins to the reference - never the device's own output.

Gate of the f64-against-f64 comparisons: |dev - host| <= 1e-9 * max(1, |host|).  Both sides are f64; the longest chain is a 49-term
(at most 128-term) DFT followed by at most 2047 arc segments, a few 1e-11 at worst by a term-count bound; 1e-9 is the tolerance the
project uses for f64 against f64.  SPARC has one discontinuity, the A_k >= 0.05 threshold: a row may be left out of the SPARC
comparison only if the HOST spectrum of that profile has a bin within 1e-9 of 0.05, at most 0.5 % of the rows, and the count is
asserted."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests.util import T, TINY_DIMS, cfgs_for
from tests.util import GATE, KEYS, MARGIN, host_metrics as _host_metrics, metrics_gate as _gate, metrics_margins as _margins, noisy_lines as _noisy_lines, threshold_margin as _threshold_margin  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
def test_g13_in_one_call(golden):
    """the six fixture trajectories as ONE batch against the reference's recorded outputs, with the tolerances
    tests/test_evaluation.py::test_metrics_against_the_reference holds the host functions to"""
    from edmp_amd import evaluation as EV

    g = golden("g13_metrics")
    dt = float(g["dt"])
    X = np.ascontiguousarray(g["trajectories"], dtype=np.float64)
    m = EV.batch_metrics(X, device=DEV, dt=dt)
    assert set(m) == set(KEYS) and all(m[k].shape == (len(X),) and m[k].dtype == np.float64 for k in KEYS)
    for i in range(len(X)):
        assert abs(m["joint_path_length"][i] - g["joint_path_length"][i]) <= 1e-9 * max(1.0, g["joint_path_length"][i]), i
        assert abs(m["ee_path_length"][i] - g["ee_path_length"][i]) <= 2e-5 * max(1.0, g["ee_path_length"][i]), i
        sj, se = m["joint_sparc"][i], m["ee_sparc"][i]
        assert abs(sj - g["joint_sparc"][i]) <= 1e-9 and abs(sj - g["third_party_joint_sparc"][i]) <= 1e-9, (i, sj, g["joint_sparc"][i])
        assert abs(se - g["ee_sparc"][i]) <= 5e-4 * max(1.0, abs(g["ee_sparc"][i])), (i, se, g["ee_sparc"][i])
    assert all(m[k][4] == 0.0 for k in KEYS)  # the constant trajectory: the reference returns 0


def test_1024_rows_against_the_host_functions():
    """Measured on an MI355X (profiles/batch_metrics_parity.json, written by this test): see that file for the four maxima."""
    from edmp_amd import evaluation as EV

    dt = 0.1
    X = _noisy_lines(1024, 50)
    dev = EV.batch_metrics(X, device=DEV, dt=dt)
    host = _host_metrics(X, dt)
    # for this input the host alone leaves out NO row (smallest margin over its 2048 profiles: 1.8e-7)
    worst, excluded, margin = _gate(dev, host, X, dt, "1024 noisy lines", max_excluded=0)
    rec = dict(test="tests/test_gpu_batch_metrics.py::test_1024_rows_against_the_host_functions", rows=1024, N=50, dt=dt, gate=GATE,
               measure="max over rows of |device - host| / max(1, |host|), host = evaluation.path_lengths / smoothness_metric",
               max_error=worst, rows_excluded_by_threshold_margin=excluded, threshold_margin=MARGIN, smallest_host_threshold_margin=margin,
               device=torch.cuda.get_device_name(0))
    with open(os.path.join(ROOT, "profiles", "batch_metrics_parity.json"), "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


def test_sampler_output_as_device_tensor():
    from edmp_amd import evaluation as EV
    from edmp_amd import scenes
    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.temporalunet import TemporalUNet

    cfgs = cfgs_for([1, 10], 32)
    B = cfgs["total_batch_size"]
    assert B == 64
    guide = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, B)
    net = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=W.init_state_dict(5, 7, 32, TINY_DIMS), max_batch=B)
    noise = np.random.RandomState(3).standard_normal((T + 1, B, 7, 50))
    Xd = Diffusion(T, DEV).denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL,
                                          noise=noise, return_device=True)
    assert Xd.is_cuda and bool(torch.isfinite(Xd).all())
    dev = guide.metrics_rows(Xd)
    X = Xd.cpu().numpy()
    _gate(dev, _host_metrics(X, 0.1), X, 0.1, "sampler output, 64 rows")
    # the same through the module-level call with device results
    d2 = EV.batch_metrics(Xd, device=DEV, return_device=True)
    assert all(d2[k].is_cuda and np.array_equal(d2[k].cpu().numpy(), dev[k]) for k in KEYS)


@pytest.mark.parametrize("N", [3, 17, 33, 65, 129])
def test_shapes(N):
    from edmp_amd import evaluation as EV

    X = _noisy_lines(64, N, seed=100 + N)
    for dt in (0.1, 0.05, 0.125):  # fs / nfft exact in binary; dt = 0.05 (fs = 20) cuts the kept bins in half
        dev = EV.batch_metrics(X, device=DEV, dt=dt)
        _gate(dev, _host_metrics(X, dt), X, dt, f"N = {N}, dt = {dt}")


def test_refused_shapes():
    from edmp_amd import _capi
    from edmp_amd import evaluation as EV

    for N, dt in ((2, 0.1), (130, 0.1), (50, 0.0), (50, float("nan")), (50, -0.1)):
        with pytest.raises(_capi.EdmpError, match="edmp_metrics_rows_dev"):
            EV.batch_metrics(np.zeros((2, 7, N)), device=DEV, dt=dt)
    with pytest.raises(ValueError):
        EV.batch_metrics(np.zeros((2, 6, 50)), device=DEV)


def test_non_finite_rows():
    from edmp_amd import evaluation as EV

    X = _noisy_lines(64, 50, seed=9)
    clean = EV.batch_metrics(X, device=DEV)
    Y = X.copy()
    Y[5, 3, 20] = np.nan
    Y[40, 2, 10] = np.inf
    got = EV.batch_metrics(Y, device=DEV)
    others = np.setdiff1d(np.arange(64), [5, 40])
    for k in KEYS:
        assert np.array_equal(got[k][others], clean[k][others]), k  # bit-equal: a row does not see its neighbours
    assert np.isnan(got["joint_sparc"][[5, 40]]).all() and np.isnan(got["ee_sparc"][[5, 40]]).all()
    with np.errstate(all="ignore"):
        for r in (5, 40):
            pl = EV.path_lengths(Y[r])
            for k, want in (("joint_path_length", pl["joint"]), ("ee_path_length", pl["end_effector"])):
                assert (np.isnan(want) and np.isnan(got[k][r])) or got[k][r] == want, (r, k, got[k][r], want)
    assert np.isnan(got["joint_path_length"][5]) and got["joint_path_length"][40] == np.inf


def test_determinism_and_row_independence():
    from edmp_amd import evaluation as EV

    X = _noisy_lines(1024, 50)
    a = EV.batch_metrics(X, device=DEV)
    b = EV.batch_metrics(torch.from_numpy(X).to(DEV), device=DEV)
    part = EV.batch_metrics(X[100:164], device=DEV)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(part[k], a[k][100:164]), k


def _selection_rows():
    """32 rows from start to goal: gentle random bows of different size (row 11 the straight line), rows 3, 17, 25 swung far down"""
    from edmp_amd import scenes

    rs = np.random.RandomState(11)
    B, N = 32, 50
    a, b = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    t = np.linspace(0, 1, N)
    X = np.tile((a[:, None] * (1 - t) + b[:, None] * t)[None], (B, 1, 1))
    amp = rs.uniform(0.02, 0.12, B)
    amp[11] = 0.0
    X += amp[:, None, None] * rs.standard_normal((B, 7, 1)) * np.sin(np.pi * t)[None, None, :]
    driven = [3, 17, 25]
    for r in driven:
        X[r, 1] += 0.9 * np.sin(np.pi * t)
    X[:, :, 0], X[:, :, -1] = a[None], b[None]
    return np.ascontiguousarray(X), driven


def _select_dev(vol, key, trust=0.0008):
    from edmp_amd import _capi
    from edmp_amd.runtime import get_context, ptr

    ctx = get_context(DEV)
    v = ctx.to_dev(np.asarray(vol, dtype=np.float32), torch.float32)
    k = ctx.to_dev(np.asarray(key, dtype=np.float64), torch.float64)
    out = C.c_int(-1)
    _capi.check(ctx.lib.edmp_select_row_dev(ctx.h, ptr(v), ptr(k), len(vol), C.c_double(trust), C.byref(out)), "edmp_select_row_dev")
    return out.value


def test_selection():
    from edmp_amd import evaluation as EV
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    X, driven = _selection_rows()
    B = len(X)
    start, goal = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    scene = scenes.random_scene(5, 6)
    scene[:, 0] += 10.0  # out of reach ...
    scene[0, :3] = EV.end_effector_positions(X[driven[0]])[25]  # ... but one box where the driven rows' hand passes
    scene[0, 3:7] = [0, 0, 0, 1]
    scene[0, 7:10] = 0.25
    guide = IntersectionVolumeGuide(scene, DEV, cfgs_for([1], B), B)
    vols, m = guide.row_swept_volumes(start, goal, X)
    # the case is what it is meant to be - checked on row_swept_volumes' own output and the host functions
    v64, trust = vols.astype(np.float64), 0.0008
    cand = np.nonzero(v64 < v64[m] + trust)[0]
    assert m == int(np.argmin(vols)) and len(cand) >= 2 and len(cand) < B and not set(driven) & set(cand.tolist())
    assert np.min(np.abs(v64 - (v64[m] + trust))) > 1e-6
    host = _host_metrics(X, 0.1)
    pl, sp = host["joint_path_length"], host["joint_sparc"]
    assert np.min(np.diff(np.sort(pl[cand]))) > 1e-6 and np.min(np.diff(np.sort(sp[cand]))) > 1e-6
    shortest, smoothest = int(cand[np.argmin(pl[cand])]), int(cand[np.argmax(sp[cand])])
    assert shortest != m and shortest == 11
    # prefer=None: the reference's rule, nothing else
    i0, v0, m0 = guide.select_row(start, goal, X)
    assert i0 == m and np.array_equal(v0, vols) and m0 is None
    assert np.array_equal(guide.choose_best_trajectory(start, goal, X), X[m])
    # the trust-region picks, host input and device input
    for Xin in (X, torch.from_numpy(X).to(DEV)):
        i1, v1, m1 = guide.select_row(start, goal, Xin, prefer="shortest")
        assert i1 == shortest and np.array_equal(v1, vols)
        assert np.abs(m1["joint_path_length"] - pl).max() <= GATE * max(1.0, pl.max()) and set(m1) == set(KEYS)
        i2, _, _ = guide.select_row(start, goal, Xin, prefer="smoothest")
        assert i2 == smoothest
    assert np.array_equal(guide.choose_best_trajectory(start, goal, X, prefer="shortest"), X[shortest])
    assert np.array_equal(guide.choose_best_trajectory(start, goal, X, prefer="smoothest"), X[smoothest])
    with pytest.raises(ValueError):
        guide.select_row(start, goal, X, prefer="cheapest")
    # a zero trust region admits no row (the comparison is strict, as in infer_serial.py:124): the arg-min row; a wide one admits the
    # driven rows too; ties on the key -> first index
    assert _select_dev(vols, pl, trust=0.0) == m
    assert _select_dev(vols, -np.arange(B, dtype=np.float64), trust=10.0) == B - 1
    assert _select_dev(vols, np.zeros(B)) == int(cand[0])
    # a NaN volume wins as it does in torch.argmin (lib/guide.py:650), whatever the key
    vn = vols.copy()
    vn[[9, 20]] = np.nan
    for key in (pl, -sp):
        assert _select_dev(vn, key) == 9
    # keys: NaN / inf rows are passed over; none finite -> the arg-min row
    kn = pl.copy()
    kn[shortest] = np.nan
    assert _select_dev(vols, kn) == int(cand[np.argsort(pl[cand])[1]])
    kn[:] = np.nan
    assert _select_dev(vols, kn) == m
    assert _select_dev(vols, np.full(B, np.inf)) == m


PARENT_RESULT_KEYS = {"scene_type", "scene_num", "timings", "best_row", "swept_volume", "success_proxy", "success_strict", "rows_collision_free", "rows_ok", "rows",
                      "aabb_volume_zero", "first_collision_waypoint", "path_length", "sparc", "planning_time_s", "scene_wall_s", "trajectory", "done_at"}
PARENT_TIMING_KEYS = {"guide_ctor_s", "ik_filter_s", "noise_wait_s", "denoise_s", "best_trajectory_s", "success_check_s"}


def test_driver(tmp_path):
    import yaml

    import infer_serial
    from edmp_amd import scenes

    guides, bpg = [1, 2, 10], 8
    cfg = {"guide": {"guides": guides, "batch_size_per_guide": bpg, "guide_path": "./guides/"},
           "dataset": {"path": "./datasets/", "dataset_type": "synthetic", "scene_types": ["stress"], "num_scenes_per_type": 2},
           "model": {"model_dir": "./models/", "device": DEV, "T": T, "traj_len": 50, "num_channels": 7}, "general": {"gui": False}}
    os.makedirs(tmp_path / "configs")
    path = str(tmp_path / "configs" / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)

    def run(**kw):
        np.random.seed(17)
        ds = scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=2, n_obstacles=6, n_cylinders=1)
        return infer_serial.run(path, dataset=ds, verbose=False, **kw)

    plain = run()
    assert len(plain) == 2
    for r in plain:  # without the flags: the parent's keys
        assert set(r) == PARENT_RESULT_KEYS and set(r["timings"]) == PARENT_TIMING_KEYS
    rep = run(ensemble_report=True)
    grp = run(ensemble_report=True, scenes_per_launch=2)
    for a, r, g in zip(plain, rep, grp):
        assert set(r) == PARENT_RESULT_KEYS | {"ensemble"}
        assert (r["best_row"], r["rows_ok"], r["rows_collision_free"]) == (a["best_row"], a["rows_ok"], a["rows_collision_free"]) and np.array_equal(r["trajectory"], a["trajectory"])
        e = r["ensemble"]
        assert [x["guide"] for x in e] == guides and [(x["first_row"], x["rows"]) for x in e] == [(0, bpg), (bpg, bpg), (2 * bpg, bpg)]
        assert sum(x["rows_collision_free"] for x in e) == r["rows_collision_free"] and sum(x["rows_ok"] for x in e) == r["rows_ok"]
        assert min(x["min_swept_volume"] for x in e) == r["swept_volume"] and r["best_row"] in [x["best_row"] for x in e]
        assert all((x["mean"] is None) == (x["rows_collision_free"] == 0) for x in e)
        assert g["ensemble"] == e and g["scenes_in_launch"] == 2  # one batch_metrics call over both scenes' rows: the same lists exactly
        json.dumps(e)
    for pref in ("shortest", "smoothest"):
        for r, a in zip(run(prefer=pref, ensemble_report=True), plain):
            assert r["prefer"] == pref and abs(r["swept_volume"] - a["swept_volume"]) < 0.0008 + 1e-12
            assert r["swept_volume"] >= a["swept_volume"]
