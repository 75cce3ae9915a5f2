"""Inputs of the scene-batch scoring tests (test infrastructure, no GPU needed): three scenes as tests/test_gpu_scene_batch.py builds
them - 4 obstacles, 16 obstacles of which 3 are true cylinders, 64 obstacles; different guide lists; B = 24 rows - and a finished state
X (S, B, 7, N) built by hand instead of by the UNet: every scene's joint-space line start -> goal plus seeded white noise at amplitudes
from 0 up to 3 rad (joint 4 spans 3.0 rad in all, so amplitude 3 certainly leaves the limits), start / goal columns pinned as the
sampler pins them.

Dataset parameters (scene number and IK-goal index per scene) are chosen so that the per-row success flags are mixed: the straight line
of every scene is collision-free, large amplitudes collide, and small amplitudes stay inside the joint limits
while large ones leave them.  tests/test_scene_score_host.py checks that choice on the CPU with oracle/success_oracle.py."""
import numpy as np

from tests.util import cfgs_for

B, N = 24, 50
#        obstacles, true cylinders, (guide list, rows per guide), scene number, IK-goal index
SPEC = [(4, 0, ([1, 5, 10], 8), 0, 0),
        (16, 3, ([11, 13], 12), 5, 1),
        (64, 0, ([13, 1, 11, 5], 6), 4, 13)]
# one exact line (row 0), then rising amplitudes; SPARE (the last row) is a second small-amplitude row the GPU tests overwrite with a
# copy of the scene's minimum row to place an exact tie
AMPS = [0.0, 1e-4, 1e-3, 3e-3, 0.01, 0.02, 0.03, 0.05, 0.08, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5, 0.7, 1.0, 1.5, 2.0, 3.0, 0.01, 0.05, 0.2, 1e-3]
SPARE = B - 1
NAN_AT = (1, 7, 3, 20)  # (scene, row, joint, waypoint): ONE row with a NaN, in the middle scene only


def scene_parts():
    """per scene: dict(obstacle_config, kinds, cfgs, guides (the guide list), start, goal)"""
    from edmp_amd.scenes import SyntheticDataset

    out = []
    for no, ncyl, (gl, bpg), scene_num, goal_idx in SPEC:
        ds = SyntheticDataset(scene_types=("stress",), num_scenes_per_type=8, n_obstacles=no, n_cylinders=ncyl)
        oc, _, _, ncub, nc, start, ik = ds.fetch_data(scene_num=scene_num, scene_type="stress")
        kinds = np.concatenate([np.zeros(int(ncub), dtype=np.int32), np.ones(int(nc), dtype=np.int32)])
        cfgs = cfgs_for(gl, bpg)
        assert cfgs["total_batch_size"] == B
        out.append(dict(obstacle_config=oc, kinds=kinds, cfgs=cfgs, guides=list(gl), start=np.asarray(start, dtype=np.float64), goal=np.asarray(ik[goal_idx], dtype=np.float64)))
    return out


def state(parts, seed=11, nan=True):
    """X (S, B, 7, N): line + AMPS[b] * N(0, 1) per scene, start / goal columns pinned; with `nan` the one NaN of NAN_AT"""
    rs = np.random.RandomState(seed)
    t = np.linspace(0, 1, N)
    amp = np.asarray(AMPS)
    X = np.empty((len(parts), B, 7, N))
    for s, p in enumerate(parts):
        a, b = p["start"], p["goal"]
        X[s] = (a[:, None] * (1 - t) + b[:, None] * t)[None] + amp[:, None, None] * rs.standard_normal((B, 7, N))
        X[s, :, :, 0], X[s, :, :, -1] = a[None], b[None]
    if nan:
        X[NAN_AT] = np.nan
    return np.ascontiguousarray(X)
