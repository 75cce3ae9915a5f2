"""Host side of the IK solver (no GPU): the seed stream, the argument checks of ik.solve / FrankaIK / SceneBatch.filter_goals' device form
(which must raise before anything touches the library), the two entry points in the header and the binding, the problem set's target
accessor, and the condition the GPU tests' inputs have to meet (tests/ik_inputs.py)."""
import os
import re

import numpy as np
import pytest

from tests import ik_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _NoGpu():
    """a context stand-in (get_context passes a Context through): any use of it means the call went past its argument checks"""
    from edmp_amd.runtime import Context

    class NoGpu(Context):
        def __init__(self):
            pass

        def __getattr__(self, name):
            raise AssertionError(f"argument checks let the call reach the context ({name})")

    return NoGpu()


def test_draw_seeds_is_private_repeatable_and_inside_the_limits():
    from edmp_amd import franka, ik

    lo, hi = franka.joint_limits()
    np.random.seed(77)
    before = np.random.get_state()
    a = ik.draw_seeds(256, 3)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]  # the global stream did not move
    assert a.shape == (256, 7) and a.dtype == np.float64
    assert np.array_equal(a, ik.draw_seeds(256, 3)) and not np.array_equal(a, ik.draw_seeds(256, 4))
    assert np.array_equal(a[:10], ik.draw_seeds(10, 3))  # a longer draw continues a shorter one
    assert (a >= lo).all() and (a <= hi).all()
    assert (a.max(axis=0) - a.min(axis=0) > 0.9 * (hi - lo)).all()  # and fills them
    start = np.array([0.1, -3.0, 0.2, -1.0, 5.0, 1.0, 0.3])  # joints 2 and 5 outside
    b = ik.draw_seeds(16, 3, start=start)
    assert np.array_equal(b[0], np.clip(start, lo, hi)) and np.array_equal(b[1:], a[1:16])
    for bad in (0, -1):
        with pytest.raises(ValueError):
            ik.draw_seeds(bad, 0)
    with pytest.raises(ValueError):
        ik.draw_seeds(4, 0, start=np.zeros(6))


def test_tool_frames():
    from edmp_amd import ik

    for name in (None, "flange", "hand"):
        assert np.array_equal(ik.tool_frame(name), I.tool_matrix(name)[:3])
    assert np.array_equal(ik.tool_frame("flange"), [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.107]])
    c = np.cos(-np.pi / 4)
    assert np.allclose(ik.tool_frame("hand")[:, :3], [[c, c, 0], [-c, c, 0], [0, 0, 1]], atol=1e-15)
    custom = I.fk(np.array([0.3, 0.2, -0.1, -1.0, 0.4, 1.2, 0.5]))
    assert np.array_equal(ik.tool_frame(custom), custom[:3]) and np.array_equal(ik.tool_frame(custom[:3]), custom[:3])
    for bad in ("right_gripper", "tcp", ""):
        with pytest.raises(ValueError, match="unknown tool"):
            ik.tool_frame(bad)


def _good():
    return I.targets()[:2], [s[:5] for s in I.seeds()[:2]]


BAD = ["targets_2d", "targets_3x3", "targets_empty", "target_nan", "target_not_orthonormal", "target_reflection", "target_last_row", "pair_shapes", "zero_quaternion",
       "seeds_count", "seeds_cols", "seeds_empty", "seeds_nan", "seeds_outside", "seeds_zero", "damping_zero", "damping_negative", "damping_nan", "iters_zero",
       "iters_fraction", "max_step_zero", "tol_negative", "tol_inf", "tool_name", "tool_shape", "tool_nan", "tool_sheared"]


@pytest.mark.parametrize("case", BAD)
def test_solve_checks_its_arguments_before_any_library_call(case):
    from edmp_amd import franka, ik

    tg, sd = _good()
    tg, sd, kw = np.array(tg), [np.array(s) for s in sd], {}
    lo, hi = franka.joint_limits()
    if case == "targets_2d":
        tg = tg[0]
    elif case == "targets_3x3":
        tg = tg[:, :3, :3]
    elif case == "targets_empty":
        tg, sd = [], []
    elif case == "target_nan":
        tg[1, 0, 3] = np.nan
    elif case == "target_not_orthonormal":
        tg[1, :3, 0] *= 1 + 1e-8
    elif case == "target_reflection":
        tg[0, :3, 2] *= -1
    elif case == "target_last_row":
        tg[0, 3, 3] = 2.0
    elif case == "pair_shapes":
        tg = [(np.zeros(3), np.array([1.0, 0, 0])), (np.zeros(3), np.array([1.0, 0, 0, 0]))]
    elif case == "zero_quaternion":
        tg = [(np.zeros(3), np.zeros(4)), (np.zeros(3), np.array([1.0, 0, 0, 0]))]
    elif case == "seeds_count":
        sd = sd[:1]
    elif case == "seeds_cols":
        sd[0] = sd[0][:, :6]
    elif case == "seeds_empty":
        sd[1] = sd[1][:0]
    elif case == "seeds_nan":
        sd[1][2, 3] = np.nan
    elif case == "seeds_outside":
        sd[0][4, 3] = hi[3] + 1e-12
    elif case == "seeds_zero":
        sd = 0
    elif case == "damping_zero":
        kw["damping"] = 0.0
    elif case == "damping_negative":
        kw["damping"] = -0.01
    elif case == "damping_nan":
        kw["damping"] = np.nan
    elif case == "iters_zero":
        kw["iters"] = 0
    elif case == "iters_fraction":
        kw["iters"] = 1.5
    elif case == "max_step_zero":
        kw["max_step"] = 0.0
    elif case == "tol_negative":
        kw["tol_pos"] = -1e-6
    elif case == "tol_inf":
        kw["tol_ang"] = np.inf
    elif case == "tool_name":
        kw["tool"] = "right_gripper"
    elif case == "tool_shape":
        kw["tool"] = np.eye(3)
    elif case == "tool_nan":
        kw["tool"] = np.full((4, 4), np.nan)
    elif case == "tool_sheared":
        t = np.eye(4)
        t[0, 1] = 1e-6
        kw["tool"] = t
    with pytest.raises(ValueError):
        ik.solve(_NoGpu(), tg, sd, **kw)


def test_the_good_arguments_pass_the_checks():
    """the counterpart of the cases above: what they start from reaches the context"""
    from edmp_amd import ik

    tg, sd = _good()
    with pytest.raises(AssertionError, match="reach the context"):
        ik.solve(_NoGpu(), tg, sd)
    pairs = [(np.array([0.4, 0.0, 0.4]), np.array([0.0, 1.0, 0.0, 0.0]))]
    with pytest.raises(AssertionError, match="reach the context"):
        ik.solve(_NoGpu(), pairs, 4, tool="hand")
    m = ik.target_matrices(pairs)
    assert m.shape == (1, 3, 4) and np.array_equal(m[0], [[1, 0, 0, 0.4], [0, -1, 0, 0.0], [0, 0, -1, 0.4]])  # a half turn about x


def test_franka_ik_checks_on_construction():
    from edmp_amd import ik

    for kw in (dict(n_seeds=0), dict(tool="gripper"), dict(damping=0.0), dict(iters=0)):
        with pytest.raises(ValueError):
            ik.FrankaIK(_NoGpu(), **kw)
    f = ik.FrankaIK(_NoGpu(), n_seeds=8, seed=5, tool="flange")
    assert f.n_seeds == 8 and f.params["iters"] == 64 and f.params["damping"] == 0.01 and f.params["max_step"] == 0.5
    assert f.params["tol_pos"] == 1e-6 and f.params["tol_ang"] == 1e-6
    with pytest.raises(ValueError):
        f((0.4, 0.0, 0.4), (0.0, 0.0, 0.0, 0.0))


def test_filter_goals_device_form_is_checked_on_the_host():
    """counts with a 0 name the scene; the device form without a device tensor, or with counts that do not tile it, is refused"""
    import torch

    from edmp_amd.guide import SceneBatch, goal_filter_device_inputs

    batch = object.__new__(SceneBatch)
    batch.__dict__.update(ctx=_NoGpu(), n_scenes=3, batch_size=4)
    starts = np.zeros((3, 7))
    with pytest.raises(ValueError, match="scene 1"):
        goal_filter_device_inputs(3, starts, torch.zeros((5, 7), dtype=torch.float64), [3, 0, 2])
    for goals, counts in ((torch.zeros((5, 7), dtype=torch.float64), [3, 1, 1]),  # a host tensor
                          (np.zeros((5, 7)), [3, 1, 1]), ([np.zeros((3, 7))] * 3, [3, 3, 3])):
        with pytest.raises(ValueError):
            batch.filter_goals(starts, goals, counts=counts)
    with pytest.raises(ValueError):
        batch.filter_goals(np.zeros((2, 7)), np.zeros((5, 7)), counts=[3, 1, 1])


def test_ik_symbols_are_declared_bound_and_exported():
    from edmp_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "edmp_hip.h")).read()
    assert "atan2" in hdr and "orthonormal" in hdr  # the header states the angle that is tested and the rotation check
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(edmp_[a-z0-9_]+)\s*\(", hdr))
    lib = _capi.load()  # dlopen works without a GPU
    for name, nargs in (("edmp_ik_solve_dev", 14), ("edmp_ik_compact_dev", 7)):
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
        assert len(_capi.SIGNATURES[name][1]) == nargs, name
    # no context: refused before anything touches a device
    assert lib.edmp_ik_solve_dev(None, None, 1, None, None, None, 64, 0.01, 0.5, 1e-6, 1e-6, None, None, None) == -1
    assert b"edmp_ik_solve_dev" in lib.edmp_last_error()
    assert lib.edmp_ik_compact_dev(None, None, None, 1, None, None, None) == -1 and b"edmp_ik_compact_dev" in lib.edmp_last_error()
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"ik.hip"' in src and '"rccl_hook.hip"' in src and '"ik.o"' in src  # built, and both sources make a stale library rebuild


def test_problem_set_target_pose_and_caller_goals(tmp_path):
    import json

    from edmp_amd import scenes

    oc = scenes.random_scene(3, 4)
    cub = [{"center": o[:3].tolist(), "quaternion_wxyz": [float(o[6]), float(o[3]), float(o[4]), float(o[5])], "dims": o[7:10].tolist()} for o in oc]
    tgt = {"xyz": [0.4, 0.1, 0.5], "quaternion_wxyz": [0.0, 1.0, 0.0, 0.0], "frame": "right_gripper"}
    own = np.random.RandomState(1).uniform(-1, 1, (3, 7))
    probs = [{"cuboids": cub, "cylinders": [], "start": [0.0] * 7, "target": tgt}, {"cuboids": cub, "cylinders": [], "start": [0.0] * 7, "target": tgt, "goals": own.tolist()},
             {"cuboids": cub, "cylinders": [], "start": [0.0] * 7}]
    p = tmp_path / "ps.json"
    json.dump({"scene_types": {"tabletop": probs}}, open(p, "w"))
    ds = scenes.ProblemSetDataset(str(p))
    xyz, quat = ds.target_pose(0, "tabletop")
    assert np.array_equal(xyz, tgt["xyz"]) and np.array_equal(quat, tgt["quaternion_wxyz"]) and xyz.dtype == np.float64
    assert ds.target_pose(1, "tabletop") is None  # carries its own goals
    with pytest.raises(ValueError, match="neither"):
        ds.target_pose(2, "tabletop")
    with pytest.raises(ValueError, match="no IK goals"):  # unchanged: no goals, no ik
        ds.fetch_data(0, "tabletop")
    given = np.random.RandomState(2).uniform(-1, 1, (5, 7))
    assert np.array_equal(ds.fetch_data(0, "tabletop", goals=given)[6], given)
    assert np.array_equal(ds.fetch_data(1, "tabletop", goals=given)[6], own)  # the file's goals win
    calls = []
    ds2 = scenes.ProblemSetDataset(str(p), ik=lambda x, q: calls.append((x, q)) or given[:2])
    assert np.array_equal(ds2.fetch_data(0, "tabletop")[6], given[:2]) and len(calls) == 1


def test_the_fixed_inputs_meet_their_condition():
    """8 targets inside the middle 70 % of every joint's range, 256 in-limit seeds each, and the NumPy restatement at the defaults finds at
    least 32 valid solutions per target - each of which passes the FK check the GPU tests apply"""
    from edmp_amd import franka

    lo, hi = franka.joint_limits()
    qs = I.target_configurations()
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    assert qs.shape == (8, 7) and (np.abs(qs - mid) <= 0.7 * half).all()
    assert I.targets().shape == (8, 4, 4) and len(I.seeds()) == 8
    counts = []
    for t, (q, res, valid) in enumerate(I.host_solutions()):
        sd = I.seeds()[t]
        assert sd.shape == (256, 7) and (sd >= lo).all() and (sd <= hi).all()
        assert max(I.pose_error(I.fk(qs[t]), I.targets()[t])) < 1e-15
        counts.append(int(valid.sum()))
        for row in q[valid][:8]:
            I.check_goal(row, I.targets()[t])
        assert np.isfinite(q).all() and (q >= lo).all() and (q <= hi).all()
    print("host restatement, valid of 256 per target:", counts)
    assert min(counts) >= I.MIN_HOST_YIELD, counts


def test_the_restatement_tells_a_half_turn_from_a_solution():
    """the angle is the true one: a pose turned by pi about the tool's x axis has a vanishing cross-product error and an angle of pi"""
    A = I.fk(I.target_configurations()[0])
    B = A.copy()
    B[:3, 1:3] *= -1
    pos, ang = I.pose_error(A, B)
    assert pos == 0.0 and abs(ang - np.pi) < 1e-12


def test_the_quaternions_of_the_fixed_targets_give_the_targets_back():
    """the end-to-end GPU test writes the targets as (xyz, quaternion_wxyz); some lie near a half turn (w near 0)"""
    from edmp_amd import ik

    ws = []
    for tg in I.targets():
        quat = I.quaternion_wxyz(tg[:3, :3])
        ws.append(abs(quat[0]))
        assert abs(np.linalg.norm(quat) - 1.0) < 1e-14
        back = np.concatenate([ik.pose_matrix(tg[:3, 3], quat), [[0.0, 0.0, 0.0, 1.0]]])
        pos, ang = I.pose_error(back, tg)
        assert pos == 0.0 and ang < 1e-14, (pos, ang)
    assert min(ws) < 0.1 < max(ws)
