"""CPU: the inputs of the IK-goal filter tests (tests/goal_filter_inputs.py) are not vacuous, and the host rule guide.pick_goal is the
three lines of the reference's filter (infer_serial.py:119-129) it replaces.  The volumes come from the restated reference
(oracle.edmp_oracle.GuideOracle.cost at t = 0); tests/test_gpu_goal_filter.py holds the device to the same inputs."""
import numpy as np
import pytest

from tests import goal_filter_inputs as GI


@pytest.fixture(scope="module")
def scenes():
    """per scene: the parts and the oracle's (MAX_M,) f32 candidate volumes; a smaller M of the same scene is a prefix"""
    from oracle import edmp_oracle as O

    parts = GI.scene_parts()
    for p in parts:
        c = p["candidates"]
        e = O.GuideOracle(p["obstacle_config"], p["cfgs"], GI.B).cost(c.reshape(-1, 7, 1), 0, batch_size=c.shape[0])
        p["volumes"] = np.asarray(e.sum(axis=(1, 2)).cpu().numpy(), dtype=np.float32)
    return parts


def _reference_lines(volumes, all_ik_goals, start_joints):
    """infer_serial.py:119-129 as the driver wrote it out"""
    indices = np.argsort(volumes)
    goal_joints = all_ik_goals[indices][volumes[indices] < np.min(volumes) + 0.0008]
    return goal_joints[np.argmin(np.linalg.norm(start_joints - goal_joints, axis=1))]


def _cases():
    return sorted({(s, c[s]) for c in GI.COUNTS for s in range(3)})


def test_a_smaller_candidate_set_is_a_prefix(scenes):
    for s, M in _cases():
        assert np.array_equal(GI.candidates(s, M), scenes[s]["candidates"][:M]), (s, M)


def test_inputs_are_not_vacuous(scenes):
    from edmp_amd.guide import pick_goal

    #         (scene, M): candidates within the trust region, pick, arg-min
    expect = {(0, 100): (73, 16, 0), (0, 300): (215, 165, 0), (1, 37): (13, 14, 1), (1, 65): (23, 14, 1), (2, 5): (1, None, None), (2, 1): (1, 0, 0)}
    interesting = set()
    for s, M in _cases():
        p = scenes[s]
        v, goals = p["volumes"][:M], p["candidates"][:M]
        assert np.isfinite(v).all() and (v >= 0).all()
        thr = float(v.min()) + GI.TRUST
        inside = v.astype(np.float64) < thr
        # NumPy's own rule on f32 volumes (the threshold rounded to f32) keeps the same rows
        assert np.array_equal(inside, v < np.float32(v.min()) + np.float32(GI.TRUST)), (s, M)
        margin = float(np.min(np.abs(v.astype(np.float64) - thr) / thr))
        idx, chosen = pick_goal(v, goals, p["start"])
        print(f"[goal filter inputs] scene {s} M={M}: {int(inside.sum())} within the trust region, min volume {v.min():.3g}, pick {idx}, "
              f"arg-min {int(np.argmin(v))}, margin to the threshold {margin:.3g}")
        assert margin >= 1e-3, (s, M, margin)  # summation rounding (<= 9 * 64 * 2^-24 = 3.4e-5 relative) cannot move a row across
        n_in, pick, amin = expect[(s, M)]
        assert int(inside.sum()) == n_in, (s, M, int(inside.sum()))
        if pick is not None:
            assert (idx, int(np.argmin(v))) == (pick, amin), (s, M, idx, int(np.argmin(v)))
        if 1 < inside.sum() < M and idx != int(np.argmin(v)):
            interesting.add(s)
        keys = np.linalg.norm(p["start"] - goals, axis=1)
        assert np.unique(keys).size == M  # all candidate keys are distinct
        assert np.array_equal(chosen, goals[idx]) and np.array_equal(chosen, _reference_lines(v, goals, p["start"])), (s, M)
    assert len(interesting) >= 2, interesting
    assert float(scenes[2]["volumes"][:5].min()) > 0.0  # scene 2: the threshold depends on the minimum


def test_pick_goal_rule_on_ties():
    """equal distances: the smaller volume wins, then the lower index; outside the trust region a nearer goal does not count"""
    from edmp_amd.guide import pick_goal

    start = np.zeros(7)
    goals = np.zeros((5, 7))
    goals[:, 0] = [2.0, 1.0, 1.0, 1.0, 0.5]
    vol = np.array([0.0, 0.0004, 0.0002, 0.0002, 0.01], dtype=np.float32)
    assert pick_goal(vol, goals, start)[0] == 2
    assert pick_goal(vol, goals, start, volume_trust_region=0.0003)[0] == 2
    assert pick_goal(vol, goals, start, volume_trust_region=0.0001)[0] == 0
    assert pick_goal(vol, goals, start, volume_trust_region=0.1)[0] == 4


def test_filter_goals_refusals_before_the_device():
    """what SceneBatch.filter_goals raises before anything is launched (guide.goal_filter_inputs, its first statement)"""
    from edmp_amd.guide import goal_filter_inputs

    rs = np.random.RandomState(0)
    starts = rs.uniform(-1, 1, (3, 7))
    goals = [rs.uniform(-1, 1, (m, 7)) for m in (4, 1, 9)]
    st, flat, counts = goal_filter_inputs(3, starts, goals)
    assert st.shape == (3, 7) and flat.shape == (14, 7) and counts.tolist() == [4, 1, 9] and counts.dtype == np.int32
    assert flat.flags.c_contiguous and flat.dtype == np.float64 and np.array_equal(flat[4], goals[1][0])
    bad = [
        (starts[:2], goals, r"starts must be \(3, 7\)"),
        (starts, goals[:2], "list of 3 arrays"),
        (starts, [goals[0], goals[1], goals[2][:, :6]], r"goals\[2\] must be \(M, 7\)"),
        (starts, [goals[0], goals[1].reshape(7), goals[2]], r"goals\[1\] must be \(M, 7\)"),
        (starts, [goals[0], np.zeros((0, 7)), goals[2]], r"goals\[1\] is empty"),
        (starts, [goals[0], goals[1], np.where(np.arange(63).reshape(9, 7) == 5, np.nan, goals[2])], r"goals\[2\] holds non-finite"),
        (starts, [np.where(np.arange(28).reshape(4, 7) == 0, np.inf, goals[0]), goals[1], goals[2]], r"goals\[0\] holds non-finite"),
        (np.where(np.arange(21).reshape(3, 7) == 8, np.nan, starts), goals, "starts holds non-finite"),
    ]
    for s, g, text in bad:
        with pytest.raises(ValueError, match=text):
            goal_filter_inputs(3, s, g)
