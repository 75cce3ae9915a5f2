"""GPU: what differs, by contract, between a single-scene scoring call and its scene-batch sibling (include/edmp_hip.h) where no other
test pins it: the single-scene entry points on a bound batch (status, a message that names the call, nothing written), the sphere
report without a table (EDMP_ERR_ARG on a guide, where the batch answers EDMP_ERR_STATE: test_gpu_scene_sdf.test_refusals), rows that
are not the bound ones at t = 0 (no smoothness weight), best-row volumes asked for without an index, and a batch of ONE scene against
its member guide.  test_gpu_scene_batch / test_gpu_scene_score / test_gpu_scene_sdf pin the status of three of the five refusals
already; here all five are held to the same three checks.

Inputs: two scenes of 2 and 3 obstacles (the last of scene 1 a true cylinder), B = 5 rows, N = 8 waypoints, no network.  Scene 0 is
five rows of the SDF guide 101 (smoothness 0.01), scene 1 one row each of guides 1, 101, 10, 13, 5."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scene_sdf_inputs as I
from tests.util import T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S, B, N = 2, 5, 8
#        obstacles, true cylinders, guide list (one row each, or B rows of one), scene number, IK-goal index
SPEC = [(2, 0, [101], 0, 0),
        (3, 1, [1, 101, 10, 13, 5], 1, 1)]
OK, ERR_ARG, ERR_STATE = 0, -1, -3


def _parts():
    from edmp_amd.scenes import SyntheticDataset

    out = []
    for no, ncyl, gl, scene_num, goal_idx in SPEC:
        ds = SyntheticDataset(scene_types=("stress",), num_scenes_per_type=3, n_obstacles=no, n_cylinders=ncyl)
        oc, _, _, ncub, nc, start, ik = ds.fetch_data(scene_num=scene_num, scene_type="stress")
        kinds = np.concatenate([np.zeros(int(ncub), dtype=np.int32), np.ones(int(nc), dtype=np.int32)])
        cfgs = I.cfgs_for(gl, B // len(gl))
        assert cfgs["total_batch_size"] == B and oc.shape[0] == no and int(kinds.sum()) == ncyl
        out.append(dict(obstacle_config=oc, kinds=kinds, cfgs=cfgs, start=np.asarray(start, dtype=np.float64), goal=np.asarray(ik[goal_idx], dtype=np.float64)))
    return out


def _state(parts, seed=3):
    """X (S, B, 7, N): every scene's joint-space line start -> goal plus white noise of amplitude 0 .. 0.4 rad, end columns pinned"""
    rs = np.random.RandomState(seed)
    t = np.linspace(0, 1, N)
    amp = np.linspace(0.0, 0.4, B)
    X = np.empty((len(parts), B, 7, N))
    for s, p in enumerate(parts):
        a, b = p["start"], p["goal"]
        X[s] = (a[:, None] * (1 - t) + b[:, None] * t)[None] + amp[:, None, None] * rs.standard_normal((B, 7, N))
        X[s, :, :, 0], X[s, :, :, -1] = a[None], b[None]
    return np.ascontiguousarray(X)


def _guide(p, cfgs=None):
    from edmp_amd.guide import IntersectionVolumeGuide

    return IntersectionVolumeGuide(p["obstacle_config"], DEV, p["cfgs"] if cfgs is None else cfgs, B, obstacle_kinds=p["kinds"])


class Data:
    def __init__(self):
        self.parts = _parts()
        self.guides = [_guide(p) for p in self.parts]
        self.starts = np.stack([p["start"] for p in self.parts])
        self.goals = np.stack([p["goal"] for p in self.parts])
        self.X = _state(self.parts)


@pytest.fixture(scope="module")
def data():
    return Data()


def _msg(lib):
    return (lib.edmp_last_error() or b"").decode()


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_single_scene_entry_points_refuse_a_bound_batch(data):
    """every single-scene sibling on a bound batch of two scenes: EDMP_ERR_STATE, a message that names the call (the best-row volumes
    go through the check they share with cost and gradient, which names the group), sentinels untouched, the batch's kinds and sphere
    table as they were"""
    from edmp_amd import _capi
    from edmp_amd.guide import SceneBatch
    from edmp_amd.runtime import ptr

    batch = SceneBatch(data.guides)
    ctx = batch.ctx
    lib, h = ctx.lib, ctx.h
    before = (batch.success_rows(data.X), batch.sdf_rows(data.X, data.starts, data.goals, 0))
    X = ctx.to_dev(data.X.reshape(S * B, 7, N), torch.float64)
    interior = ctx.to_dev(data.X.reshape(S * B, 7, N)[:, :, 1:-1], torch.float64)
    flags = ctx.empty((3, S * B), torch.int32)
    flags.fill_(-7)
    vols = ctx.empty((S * B,), torch.float32)
    vols.fill_(float("nan"))
    rep = ctx.empty((2, S * B), torch.float64)
    rep.fill_(float("nan"))
    ctx.sync()
    counts, idx = (C.c_int32 * 4)(*([-7] * 4)), C.c_int(-7)
    pd, pf, pi = _capi.as_pd, _capi.as_pf, _capi.as_pi32
    s0, g0 = np.ascontiguousarray(data.starts[0]), np.ascontiguousarray(data.goals[0])
    fl = [C.c_void_p(flags[i].data_ptr()) for i in range(3)]
    rp = [C.c_void_p(rep[i].data_ptr()) for i in range(2)]
    sdf = data.guides[0]._sdf
    kinds = np.ones(3, dtype=np.int32)
    n = S * B
    batch._bind()
    calls = [
        ("edmp_success_rows_dev", lambda: lib.edmp_success_rows_dev(h, ptr(X), n, N, 4, None, *fl, counts)),
        ("edmp_scene_set_shapes", lambda: lib.edmp_scene_set_shapes(h, pi(kinds), 3)),
        ("best-trajectory entry point", lambda: lib.edmp_row_swept_volumes_dev(h, ptr(X), n, N, pd(s0), pd(g0), ptr(vols), C.byref(idx))),
        ("edmp_sdf_rows_dev", lambda: lib.edmp_sdf_rows_dev(h, ptr(interior), n, N - 2, 0, pd(s0), pd(g0), *rp)),
        ("edmp_sdf_set", lambda: lib.edmp_sdf_set(h, pf(sdf["spheres"]), int(sdf["spheres"].shape[0]), pi(np.zeros(n, dtype=np.int32)), pd(np.zeros((n, T))),
                                                  pd(np.zeros(n)), n, T)),
    ]
    for name, call in calls:
        rc = call()
        msg = _msg(lib)
        assert rc == ERR_STATE and name in msg and f"scene batch of {S} scenes" in msg, (name, rc, msg)
    ctx.sync()
    assert (flags == -7).all().item() and torch.isnan(vols).all().item() and torch.isnan(rep).all().item()
    assert list(counts) == [-7] * 4 and idx.value == -7
    assert ctx.bound_guide is batch
    after = (batch.success_rows(data.X), batch.sdf_rows(data.X, data.starts, data.goals, 0))
    assert _same(before[0], after[0]) and _same(before[1], after[1])


def test_sphere_report_of_a_guide_without_a_table(data):
    """edmp_sdf_rows_dev on a single-scene guide that never had a sphere table: EDMP_ERR_ARG, the message says what to call, nothing is
    written"""
    from edmp_amd import _capi
    from edmp_amd.runtime import ptr

    p = data.parts[1]
    plain = _guide(p, I.without_sdf(p["cfgs"]))
    assert plain._sdf is None
    ctx = plain.ctx
    plain._bind()
    interior = ctx.to_dev(data.X[1][:, :, 1:-1], torch.float64)
    rep = ctx.empty((2, B), torch.float64)
    rep.fill_(float("nan"))
    ctx.sync()
    rc = ctx.lib.edmp_sdf_rows_dev(ctx.h, ptr(interior), B, N - 2, 0, _capi.as_pd(np.ascontiguousarray(p["start"])), _capi.as_pd(np.ascontiguousarray(p["goal"])),
                                   C.c_void_p(rep[0].data_ptr()), C.c_void_p(rep[1].data_ptr()))
    msg = _msg(ctx.lib)
    assert rc == ERR_ARG and msg.startswith("edmp_sdf_rows_dev") and "edmp_sdf_set first" in msg, (rc, msg)
    ctx.sync()
    assert torch.isnan(rep).all().item()


def test_rows_that_are_not_the_bound_ones_carry_no_smoothness(data):
    """edmp_sdf_rows_dev with n != B at t = 0 is accepted and its costs are those of a guide whose smoothness is zero everywhere"""
    p, g = data.parts[0], data.guides[0]
    zero = dict(p["cfgs"])
    zero["smoothness"] = np.zeros_like(np.asarray(p["cfgs"]["smoothness"]))
    assert np.all(np.asarray(p["cfgs"]["smoothness"]) > 0)
    gz = _guide(p, zero)
    Xi = data.X[0][:, :, 1:-1]
    full, full_z = g.sdf_rows(Xi, p["start"], p["goal"], 0), gz.sdf_rows(Xi, p["start"], p["goal"], 0)
    assert np.all(full["cost"] > full_z["cost"])  # (the weight does count when the rows are the bound ones)
    for rows in (slice(0, 3), slice(1, 2)):
        sub = g.sdf_rows(Xi[rows], p["start"], p["goal"], 0)
        assert sub["cost"].shape == (len(Xi[rows]),)
        assert np.array_equal(sub["cost"], full_z["cost"][rows]) and np.array_equal(sub["clearance"], full["clearance"][rows]), rows


def test_best_row_volumes_without_an_index(data):
    """edmp_row_swept_volumes_dev with neither a volume buffer nor an index succeeds (the volumes stay in the guide's scratch); a
    following call with both gives the first arg-min of the volumes it returns"""
    from edmp_amd import _capi
    from edmp_amd.runtime import ptr

    p, g = data.parts[1], data.guides[1]
    ctx = g.ctx
    g._bind()
    X = ctx.to_dev(data.X[1], torch.float64)
    s, gl = _capi.as_pd(np.ascontiguousarray(p["start"])), _capi.as_pd(np.ascontiguousarray(p["goal"]))
    rc = ctx.lib.edmp_row_swept_volumes_dev(ctx.h, ptr(X), B, N, s, gl, None, None)
    assert rc == OK, (rc, _msg(ctx.lib))
    vols = ctx.empty((B,), torch.float32)
    idx = C.c_int(-1)
    rc = ctx.lib.edmp_row_swept_volumes_dev(ctx.h, ptr(X), B, N, s, gl, ptr(vols), C.byref(idx))
    assert rc == OK, (rc, _msg(ctx.lib))
    vh = ctx.to_host(vols)
    assert np.isfinite(vh).all() and idx.value == int(np.argmin(vh))
    ref, ref_idx = g.row_swept_volumes(p["start"], p["goal"], data.X[1])
    assert np.array_equal(vh, ref) and idx.value == ref_idx


@pytest.mark.parametrize("s", range(S))
def test_a_batch_of_one_scene_scores_as_its_member(data, s):
    """SceneBatch([guide]) against the guide itself: best-row volumes and index, the "shortest" pick, success and the sphere report"""
    from edmp_amd.guide import SceneBatch

    g, Xs, st, gl = data.guides[s], data.X[s], data.starts[s], data.goals[s]
    ref_vols, ref_idx = g.row_swept_volumes(st, gl, Xs)
    ref_pick = g.select_row(st, gl, Xs, prefer="shortest")
    ref_chk = g.success_rows(Xs)
    ref_rep = g.sdf_rows(Xs[:, :, 1:-1], st, gl, 0)
    one = SceneBatch([g])
    vols, idx = one.row_swept_volumes(st[None], gl[None], Xs)
    assert vols.shape == (1, B) and np.array_equal(vols[0], ref_vols) and idx.tolist() == [ref_idx]
    pick, pvols, met = one.select_rows(st[None], gl[None], Xs, prefer="shortest")
    assert pick.tolist() == [ref_pick[0]] and np.array_equal(pvols[0], ref_pick[1])
    assert set(met) == set(ref_pick[2]) and all(np.array_equal(met[k][0], ref_pick[2][k]) for k in met)
    chk = one.success_rows(Xs)
    for k in ("ok", "first", "within", "collision_free"):
        assert np.array_equal(chk[k][0], ref_chk[k]), k
    for k in ("rows_ok", "rows_within", "rows_collision_free", "rows"):
        assert chk[k].tolist() == [ref_chk[k]], k
    rep = one.sdf_rows(Xs, st[None], gl[None], 0)
    assert np.array_equal(rep["cost"][0], ref_rep["cost"]) and np.array_equal(rep["clearance"][0], ref_rep["clearance"])
    assert np.isfinite(ref_rep["cost"]).all() and np.isfinite(ref_vols).all() and ref_chk["rows"] == B
