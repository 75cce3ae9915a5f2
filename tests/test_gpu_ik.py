"""GPU: the batched IK of the Franka (edmp_ik_solve_dev / edmp_ik_compact_dev, csrc/ik.hip; edmp_amd.ik) and what consumes it
(SceneBatch.filter_goals' device form, infer_serial.run(ik_seeds=...)).

The reference is not the code under test: tests/ik_inputs.py holds an f64 FK written from evaluation._dh / franka.DH_A_D_ALPHA /
EE_STATIC_DH and a NumPy restatement of the iteration; tests/test_ik_host.py checks on the CPU that the restatement finds at least 32
solutions per target from these seeds.  Every goal the GPU returns must reproduce its target under that FK.  The iteration itself is
compared step by step in tests/test_gpu_ik_steps.py."""
import json
import os

import numpy as np
import pytest

from tests import ik_inputs as I

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def full():
    """the 8 targets x 256 seeds at the defaults, solved once: host goals + per-seed outputs"""
    from edmp_amd import ik

    return ik.solve(DEV, I.targets(), I.seeds(), return_all=True)


def test_every_goal_is_a_solution_in_seed_order(full):
    from edmp_amd import franka

    lo, hi = franka.joint_limits()
    q, res, valid = full["q"], full["residuals"], full["valid"]
    assert q.shape == (8 * 256, 7) and res.shape == (8 * 256, 2) and valid.shape == (8 * 256,) and valid.dtype == bool
    assert np.array_equal(full["n_seeds"], [256] * 8) and full["counts"].dtype == np.int32
    assert np.isfinite(q).all() and (q >= lo).all() and (q <= hi).all()  # every seed ends inside the limits, valid or not
    assert np.array_equal(valid, np.isfinite(res).all(axis=1) & (res[:, 0] <= I.TOL_POS) & (res[:, 1] <= I.TOL_ANG))
    for t in range(8):
        seg = slice(256 * t, 256 * (t + 1))
        goals = full["goals"][t]
        assert full["counts"][t] == valid[seg].sum() == goals.shape[0]
        assert np.array_equal(goals, q[seg][valid[seg]])  # bit for bit, in seed order
        for g in goals:
            I.check_goal(g, I.targets()[t])
        # the residuals the kernel reports are the ones the host FK sees, to the last bits of sincos
        for r in np.flatnonzero(valid[seg])[:4]:
            pos, ang = I.pose_error(I.fk(q[seg][r]), I.targets()[t])
            assert abs(pos - res[seg][r, 0]) <= 1e-12 and abs(ang - res[seg][r, 1]) <= 1e-9


def test_yield_against_the_numpy_restatement(full):
    """per target at least one solution and at least half as many as the restatement finds from the same seeds.  Per seed, two correct
    f64 formulations agree through 16 iterations (to 3e-13 rad after one step, 8e-11 after 16, over all 2048 seeds:
    tests/ik_reference.floors) - that agreement is what tests/test_gpu_ik_steps.py holds the kernel to; by 64 iterations the steps far
    from a solution have amplified the rounding so far that 91 of the 2048 rows end more than 1e-9 apart, some on another branch,
    so at the default iteration count only the RATE is compared here: the binomial spread at 256 seeds is 7-8 seeds and half the host
    count is more than four spreads below it at the lowest yield"""
    host = [int(v.sum()) for _, _, v in I.host_solutions()]
    gpu = [int(c) for c in full["counts"]]
    print("valid of 256 seeds per target: gpu", gpu, "host restatement", host)
    for g, h in zip(gpu, host):
        assert g >= 1 and 2 * g >= h, (gpu, host)


RAGGED = [(1, 63, 64), (65, 129, 1), (64, 65, 63), (129, 1, 65), (63, 64, 129)]


@pytest.fixture(scope="module")
def alone():
    """target t (0..2) solved alone from its first n seeds, per (t, n) of RAGGED - computed once"""
    from edmp_amd import ik

    out = {}
    for counts in RAGGED:
        for t, n in enumerate(counts):
            if (t, n) not in out:
                out[(t, n)] = ik.solve(DEV, I.targets()[t:t + 1], [I.seeds()[t][:n]], return_all=True)
    return out


@pytest.mark.parametrize("counts", RAGGED)
def test_ragged_groups_equal_each_target_alone_and_repeat(alone, counts):
    """1, 63, 64, 65 and 129 seeds: the lane, wave and block boundaries of a 64-wide block, in every position of the group"""
    from edmp_amd import ik

    sd = [I.seeds()[t][:n] for t, n in enumerate(counts)]
    a = ik.solve(DEV, I.targets()[:3], sd, return_all=True)
    b = ik.solve(DEV, I.targets()[:3], sd, return_all=True)
    off = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(a["n_seeds"], counts) and a["q"].shape == (off[-1], 7)
    for k in ("q", "residuals", "valid", "counts"):
        assert np.array_equal(a[k], b[k]), k
    for t, n in enumerate(counts):
        one = alone[(t, n)]
        seg = slice(off[t], off[t + 1])
        assert np.array_equal(a["q"][seg], one["q"]) and np.array_equal(a["residuals"][seg], one["residuals"]) and np.array_equal(a["valid"][seg], one["valid"])
        assert a["counts"][t] == one["counts"][0] and np.array_equal(a["goals"][t], one["goals"][0]) and np.array_equal(b["goals"][t], one["goals"][0])
        assert np.array_equal(a["goals"][t], a["q"][seg][a["valid"][seg]])


def test_a_seed_that_solves_its_target_is_a_fixed_point():
    from edmp_amd import ik

    qs = I.target_configurations()
    r = ik.solve(DEV, I.targets(), [q[None] for q in qs], return_all=True)
    assert r["valid"].all() and np.array_equal(r["counts"], [1] * 8)
    assert np.max(np.abs(r["q"] - qs)) <= 1e-9 and np.max(r["residuals"]) < 1e-12, (np.max(np.abs(r["q"] - qs)), r["residuals"].max(axis=0))


def test_unreachable_target():
    """2 m from the base: count 0 and no error from solve, a ValueError naming the target from the callable"""
    from edmp_amd import ik

    far = np.eye(4)
    far[:3, 3] = [2.0, 0.0, 0.3]
    r = ik.solve(DEV, np.stack([I.targets()[0], far]), [I.seeds()[0][:65], I.seeds()[1][:65]], return_all=True)
    assert r["counts"][1] == 0 and r["goals"][1].shape == (0, 7) and not r["valid"][65:].any()
    assert r["counts"][0] == r["valid"][:65].sum() >= 1 and np.isfinite(r["q"]).all() and np.isfinite(r["residuals"]).all()
    assert (r["residuals"][65:, 0] > 0.5).all()
    f = ik.FrankaIK(DEV, n_seeds=64, seed=1)
    with pytest.raises(ValueError, match="target 0"):
        f(far[:3, 3], np.array([1.0, 0.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="target 1"):
        f.solve_many(np.stack([I.targets()[0], far]))
    d = ik.solve(DEV, far[None], 64, return_device=True)
    assert d["counts"][0] == 0 and tuple(d["goals"].shape) == (0, 7)


def test_degenerate_target_gives_finite_outputs():
    """joint 4 at its upper limit, the arm near full stretch (a singular Jacobian at the solution, on the boundary of the limits): every
    output is finite, and a row is either a solution under the FK check or flagged invalid"""
    from edmp_amd import franka, ik

    lo, hi = franka.joint_limits()
    q0 = np.array([0.3, 0.4, -0.2, hi[3], 0.1, 1.0, 0.5])
    tg = I.fk(q0)
    r = ik.solve(DEV, tg[None], [I.seeds()[2]], return_all=True)
    assert np.isfinite(r["q"]).all() and np.isfinite(r["residuals"]).all()
    assert (r["q"] >= lo).all() and (r["q"] <= hi).all()
    print("degenerate target: valid", int(r["valid"].sum()), "of 256")
    for row, v, res in zip(r["q"], r["valid"], r["residuals"]):
        if v:
            I.check_goal(row, tg)
        else:
            assert res[0] > I.TOL_POS or res[1] > I.TOL_ANG


def test_tool_frames():
    """the same configuration's pose under each tool frame is solved with that frame and checked with it"""
    from edmp_amd import ik

    q0 = I.target_configurations()[3]
    custom = np.eye(4)
    c, s = np.cos(0.7), np.sin(0.7)
    custom[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    custom[:3, 3] = [0.02, -0.03, 0.15]
    poses = {}
    for name, tool in (("none", None), ("flange", "flange"), ("hand", "hand"), ("custom", custom)):
        tg = I.fk(q0, tool)
        poses[name] = tg
        r = ik.solve(DEV, tg[None], [I.seeds()[3][:128]], tool=tool)
        assert r["counts"][0] >= 1, name
        for g in r["goals"][0]:
            I.check_goal(g, tg, tool)
    assert np.linalg.norm(poses["none"][:3, 3] - poses["flange"][:3, 3]) > 0.1  # the frames differ: a mix-up could not pass
    g = ik.solve(DEV, poses["hand"][None], [I.seeds()[3][:128]], tool="hand")["goals"][0][0]
    pos, ang = I.pose_error(I.fk(g, "flange"), poses["hand"])
    assert ang > 0.7


def test_c_abi_refusals():
    """edmp_ik_solve_dev's own argument checks: refused with EDMP_ERR_ARG, the outputs untouched"""
    import ctypes as C

    import torch

    from edmp_amd import _capi, ik
    from edmp_amd.runtime import get_context, ptr

    ctx = get_context(DEV)
    tg = np.ascontiguousarray(I.targets()[:2, :3].reshape(2, 12))
    tool = np.ascontiguousarray(ik.tool_frame(None).reshape(12))
    sd = ctx.to_dev(np.concatenate([I.seeds()[0][:5], I.seeds()[1][:3]]), torch.float64)
    q = torch.full((8, 7), -7.0, dtype=torch.float64, device=DEV)
    res = torch.full((8, 2), -7.0, dtype=torch.float64, device=DEV)
    valid = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def call(targets=tg, T=2, counts=(5, 3), tool_=tool, iters=64, lam=0.01, step=0.5, tp=1e-6, ta=1e-6, null_q=False):
        cn = np.asarray(counts, dtype=np.int32)
        return ctx.lib.edmp_ik_solve_dev(ctx.h, _capi.as_pd(targets), T, _capi.as_pi32(cn), ptr(sd), _capi.as_pd(tool_), iters, C.c_double(lam), C.c_double(step),
                                         C.c_double(tp), C.c_double(ta), None if null_q else ptr(q), ptr(res), ptr(valid))

    bad_t = tg.copy()
    bad_t[1, 0] += 1e-3
    nan_t = tg.copy()
    nan_t[0, 3] = np.nan
    bad_tool = tool.copy()
    bad_tool[5] += 1e-3
    for kw in (dict(T=0), dict(counts=(5, 0)), dict(iters=0), dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan")), dict(step=0.0), dict(tp=float("inf")),
               dict(ta=-1.0), dict(targets=bad_t), dict(targets=nan_t), dict(tool_=bad_tool), dict(null_q=True)):
        assert call(**kw) == -1 and b"edmp_ik_solve_dev" in ctx.lib.edmp_last_error(), kw
    cn = np.asarray([5, 0], dtype=np.int32)
    counts = np.full(2, -7, dtype=np.int32)
    assert ctx.lib.edmp_ik_compact_dev(ctx.h, ptr(q), ptr(valid), 2, _capi.as_pi32(cn), ptr(res), _capi.as_pi32(counts)) == -1
    ctx.sync()
    assert (q == -7.0).all() and (res == -7.0).all() and (valid == -7).all() and (counts == -7).all()
    assert call() == 0
    assert (valid.cpu() >= 0).all()


def test_device_goals_go_into_the_goal_filter():
    """filter_goals on solve(..., return_device=True) for a 3-scene batch: indices, chosen goals and volumes bit-identical to passing the
    same goals as host arrays"""
    import torch

    from edmp_amd import ik
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch
    from tests import goal_filter_inputs as GI

    parts = GI.scene_parts()
    batch = SceneBatch([IntersectionVolumeGuide(p["obstacle_config"], DEV, p["cfgs"], GI.B, obstacle_kinds=p["kinds"], bind=False) for p in parts])
    starts = np.stack([p["start"] for p in parts])
    sd = [I.seeds()[t][:n] for t, n in enumerate((256, 100, 65))]
    dev = ik.solve(DEV, I.targets()[:3], sd, return_device=True)
    host = ik.solve(DEV, I.targets()[:3], sd)
    assert isinstance(dev["goals"], torch.Tensor) and dev["goals"].is_cuda and np.array_equal(dev["counts"], host["counts"]) and (host["counts"] >= 2).all()
    assert np.array_equal(dev["goals"].cpu().numpy(), np.concatenate(host["goals"]))
    i_d, g_d, v_d = batch.filter_goals(starts, dev["goals"], counts=dev["counts"])
    i_h, g_h, v_h = batch.filter_goals(starts, host["goals"])
    assert np.array_equal(i_d, i_h) and np.array_equal(g_d, g_h) and g_d.dtype == np.float64
    assert len(v_d) == 3 and all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(v_d, v_h))
    for s in range(3):
        assert np.array_equal(g_d[s], host["goals"][s][i_d[s]])
        I.check_goal(g_d[s], I.targets()[s])
    zero = dev["counts"].copy()
    zero[2] = 0
    with pytest.raises(ValueError, match="scene 2"):
        batch.filter_goals(starts, dev["goals"], counts=zero)


def test_infer_serial_plans_a_problem_set_from_its_target_poses(tmp_path):
    """a problem-set JSON without `goals` (targets from FK, in the reference's end-effector frame) through infer_serial.run with ik_seeds,
    serial and two scenes per launch: each scene's chosen goal - the pinned last column of its plan - reproduces its target; without the
    flag the same file raises the existing ValueError"""
    import yaml

    import infer_serial
    from edmp_amd import franka, scenes

    lo, hi = franka.joint_limits()
    rs = np.random.RandomState(9)
    problems = []
    for k in range(2):
        oc = scenes.random_scene(20 + k, 6)
        to_wxyz = lambda o: [float(o[6]), float(o[3]), float(o[4]), float(o[5])]  # noqa: E731
        tg = I.targets()[k]
        quat = I.quaternion_wxyz(tg[:3, :3])
        problems.append({"cuboids": [{"center": o[:3].tolist(), "quaternion_wxyz": to_wxyz(o), "dims": o[7:10].tolist()} for o in oc[:4]],
                         "cylinders": [{"center": o[:3].tolist(), "quaternion_wxyz": to_wxyz(o), "radius": float(o[7]), "height": float(o[9])} for o in oc[4:]],
                         "start": rs.uniform(lo, hi).tolist(), "target": {"xyz": tg[:3, 3].tolist(), "quaternion_wxyz": quat, "frame": "end_effector"}})
    pj = tmp_path / "problems.json"
    json.dump({"format": "edmp_amd problem set v1", "scene_types": {"tabletop": problems}}, open(pj, "w"))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cfg_c1_plumbing.yaml")))
    cfg["dataset"]["scene_types"] = ["tabletop"]
    os.makedirs(tmp_path / "cfgs")
    cj = tmp_path / "cfgs" / "cfg_problem_set.yaml"
    yaml.safe_dump(cfg, open(cj, "w"))
    ds = scenes.ProblemSetDataset(str(pj))
    with pytest.raises(ValueError, match="no IK goals"):
        infer_serial.run(str(cj), dataset=ds, verbose=False)
    state = np.random.get_state()
    serial = infer_serial.run(str(cj), dataset=ds, verbose=False, ik_seeds=128)
    np.random.set_state(state)
    grouped = infer_serial.run(str(cj), dataset=ds, verbose=False, ik_seeds=128, scenes_per_launch=2)
    for res in (serial, grouped):
        assert len(res) == 2
        for k, r in enumerate(res):
            assert np.isfinite(r["trajectory"]).all() and np.array_equal(r["trajectory"][:, 0], np.asarray(problems[k]["start"]))
            I.check_goal(r["trajectory"][:, -1], I.targets()[k])
    # and the callable alone, plugged into the dataset
    from edmp_amd.ik import FrankaIK

    goals = scenes.ProblemSetDataset(str(pj), ik=FrankaIK(DEV, n_seeds=128)).fetch_data(1, "tabletop")[6]
    assert goals.ndim == 2 and goals.shape[1] == 7 and goals.shape[0] >= 1
    assert any(np.array_equal(serial[1]["trajectory"][:, -1], g) for g in goals)
