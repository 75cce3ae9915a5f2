"""Host side of scene-batch scoring (no GPU): the inputs of tests/test_gpu_scene_score.py are not vacuous - checked with the CPU
checker oracle/success_oracle.py on the same construction - and SceneBatch's scoring methods reject bad arguments before they touch
the GPU."""
import numpy as np
import pytest
import torch

from tests import scene_score_inputs as I


def test_state_construction_has_mixed_success_flags():
    """collision-free and colliding rows, rows inside and outside the joint limits, in every one of the three scenes (the GPU tests
    ask for at least two); the cylinders of the middle scene change at least one row; the NaN sits in one row of one scene"""
    from oracle import success_oracle as SO

    parts = I.scene_parts()
    assert [p["obstacle_config"].shape[0] for p in parts] == [4, 16, 64] and [int(p["kinds"].sum()) for p in parts] == [0, 3, 0]
    assert len({tuple(np.asarray(p["cfgs"]["guidance_method"]).tolist()) for p in parts}) == 3  # different guide lists
    X = I.state(parts)
    assert X.shape == (3, I.B, 7, I.N)
    assert np.isnan(X).any(axis=(2, 3)).sum(axis=1).tolist() == [0, 1, 0]
    Xf = I.state(parts, nan=False)
    assert np.array_equal(np.isnan(X), np.arange(X.size).reshape(X.shape) == np.ravel_multi_index(I.NAN_AT, X.shape))
    assert np.array_equal(X[~np.isnan(X)], Xf[~np.isnan(X)])
    for s, p in enumerate(parts):
        assert np.array_equal(Xf[s, 0], p["start"][:, None] * (1 - np.linspace(0, 1, I.N)) + p["goal"][:, None] * np.linspace(0, 1, I.N))
        r = SO.success_rows(X[s], p["obstacle_config"], substeps=4, kinds=p["kinds"])
        free = r["first"] < 0
        assert free.any() and not free.all(), (s, free)
        assert r["within"].any() and not r["within"].all(), (s, r["within"])
        assert free[0] and r["within"][0]  # the exact line is a valid plan
        assert not r["within"][np.argmax(I.AMPS)]  # the largest amplitude certainly leaves the limits
    as_boxes = SO.success_rows(X[1], parts[1]["obstacle_config"], substeps=4, kinds=None)
    as_cyl = SO.success_rows(X[1], parts[1]["obstacle_config"], substeps=4, kinds=parts[1]["kinds"])
    assert (as_boxes["first"] != as_cyl["first"]).any()


class _NoGpu:
    """a context stand-in: any use of it means the call went past its argument checks"""

    def __getattr__(self, name):
        raise AssertionError(f"argument checks let the call reach the context ({name})")


def _fake_batch(S=3, B=4, n_obstacles=(2, 5, 3)):
    from edmp_amd.guide import SceneBatch

    batch = object.__new__(SceneBatch)
    batch.__dict__.update(ctx=_NoGpu(), n_scenes=S, batch_size=B, tables=dict(n_obstacles=np.asarray(n_obstacles, dtype=np.int32)), _kinds=None)
    return batch


@pytest.mark.parametrize("case", ["rows", "scenes", "joints", "ndim", "tensor", "starts_shape", "goals_missing", "prefer", "kinds_length", "kinds_value",
                                  "kinds_per_scene"])
def test_scene_batch_scoring_checks_arguments_first(case):
    S, B, N = 3, 4, 50
    batch = _fake_batch(S, B)
    X, st, gl = np.zeros((S, B, 7, N)), np.zeros((S, 7)), np.zeros((S, 7))
    calls = [lambda X, st, gl: batch.row_swept_volumes(st, gl, X), lambda X, st, gl: batch.select_rows(st, gl, X, prefer="shortest"),
             lambda X, st, gl: batch.choose_best_trajectories(st, gl, X), lambda X, st, gl: batch.success_rows(X)]
    if case == "rows":
        X = np.zeros((S, B + 1, 7, N))
    elif case == "scenes":
        X = np.zeros(((S - 1) * B, 7, N))
    elif case == "joints":
        X = np.zeros((S, B, 6, N))
    elif case == "ndim":
        X = np.zeros((S * B * 7, N))
    elif case == "tensor":
        X = torch.zeros((S, B, 7))
    elif case == "starts_shape":
        st, calls = np.zeros((S, 6)), calls[:3]
    elif case == "goals_missing":
        gl, calls = None, calls[:3]
    elif case == "prefer":
        calls = [lambda X, st, gl: batch.select_rows(st, gl, X, prefer="longest")]
    elif case == "kinds_length":
        calls = [lambda X, st, gl: batch.set_obstacle_kinds(np.zeros(9, dtype=np.int32))]
    elif case == "kinds_value":
        calls = [lambda X, st, gl: batch.set_obstacle_kinds([0] * 9 + [2])]
    elif case == "kinds_per_scene":
        calls = [lambda X, st, gl: batch.set_obstacle_kinds([np.zeros(2), np.zeros(5), np.zeros(4)])]
    for call in calls:
        with pytest.raises(ValueError):
            call(X, st, gl)
    assert batch._kinds is None
    # a well-formed kinds array passes the check (and only then reaches the context)
    assert batch._check_kinds([np.zeros(2), np.ones(5), np.zeros(3)]).tolist() == [0, 0, 1, 1, 1, 1, 1, 0, 0, 0]
