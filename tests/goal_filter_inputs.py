"""Inputs of the IK-goal filter tests (test infrastructure, no GPU needed): the three scenes of tests/scene_score_inputs.SPEC - 4, 16
and 64 obstacles - each with the IK candidates its own SyntheticDataset(..., n_ik=M) hands out.  A case is (scene order, candidate
count per scene): the count sets (300, 37, 5) and (100, 65, 1) over scenes (0, 1, 2), and the same scenes with the same counts in the
order (2, 1, 0).  Together they hold a scene that crosses a 256-thread workgroup (300), scenes that cross a wave (65, 100), scene offsets
that are no multiple of 64, a scene with ONE candidate, and the widest obstacle table in the first and in the last position.

tests/test_goal_filter_host.py checks on the CPU that these inputs are not vacuous: the trust region keeps some rows and drops others,
the pick is not the arg-min, and no volume lies near its threshold."""
import numpy as np

from tests import scene_score_inputs as I

B = I.B
TRUST = 0.0008
COUNTS = ({0: 300, 1: 37, 2: 5}, {0: 100, 1: 65, 2: 1})
ORDERS = ((0, 1, 2), (2, 1, 0))
# (scene order, counts in that order)
CASES = [(order, tuple(c[s] for s in order)) for c in COUNTS for order in ORDERS]
MAX_M = {s: max(c[s] for c in COUNTS) for s in range(3)}


def scene_parts():
    """scene_score_inputs.scene_parts() plus `candidates`: the scene's (MAX_M, 7) IK goals"""
    parts = I.scene_parts()
    for s, p in enumerate(parts):
        p["candidates"] = candidates(s, MAX_M[s])
    return parts


def candidates(scene, M):
    """the (M, 7) IK candidates of scene `scene` as its dataset hands them out with n_ik = M"""
    from edmp_amd.scenes import SyntheticDataset

    no, ncyl, _, scene_num, _ = I.SPEC[scene]
    ds = SyntheticDataset(scene_types=("stress",), num_scenes_per_type=8, n_obstacles=no, n_cylinders=ncyl, n_ik=int(M))
    return np.ascontiguousarray(np.asarray(ds.fetch_data(scene_num=scene_num, scene_type="stress")[6], dtype=np.float64))


def ordered_sum(elements, no):
    """(M, 9 * no) element volumes -> (M,) f32: float32( sum over links ( sum over obstacles, f64 ) ), both sums sequential in index
    order in a Python loop - the order edmp_scenes_goal_filter_dev states"""
    e = np.asarray(elements).reshape(-1, 9, no)
    out = np.empty(e.shape[0], dtype=np.float32)
    for r in range(e.shape[0]):
        tot = 0.0
        for l in range(9):
            acc = 0.0
            for ob in range(no):
                acc += float(e[r, l, ob])
            tot += acc
        out[r] = np.float32(tot)
    return out
