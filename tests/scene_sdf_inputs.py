"""Inputs of the scene-batch tests of the sphere signed-distance guide (test infrastructure, no GPU needed): three scenes with 4, 9 (2
true cylinders) and 16 obstacles, their own starts / goals, and ensembles that put guide 101 at different places with different block
sizes - (1, 101, 10) x 4, (101, 13) x 6, (5, 101) x 6 - so that the SDF masks differ from scene to scene and scene 1 mixes SDF rows with
rows that normalise by the whole scene's ||g|| (guide 13)."""
import numpy as np

from edmp_amd import guide_cfg as GC
from tests.util import T

S, B, N = 3, 12, 50
#        obstacles, true cylinders, (guide list, rows per guide), scene number, IK-goal index
SPEC = [(4, 0, ([1, 101, 10], 4), 0, 0),
        (9, 2, ([101, 13], 6), 1, 1),
        (16, 0, ([5, 101], 6), 2, 2)]
SDF_KEYS = ("sdf_rows", "sdf_margin", "smoothness")
NOISE_SEED = 2024


def cfgs_for(guides, bpg):
    return GC.build_guide_cfgs([GC.load_guide_dict(int(n)) for n in guides], int(bpg), T)


def without_sdf(cfgs):
    """the guide_cfgs without the SDF keys: the guide's rows fall back to their volume gradient"""
    return {k: v for k, v in cfgs.items() if k not in SDF_KEYS}


def zero_mask(cfgs):
    """the guide_cfgs with the SDF keys kept and no row marked"""
    out = dict(cfgs)
    out["sdf_rows"] = np.zeros_like(np.asarray(cfgs["sdf_rows"]))
    return out


def scene_parts():
    """per scene: dict(obstacle_config, kinds, cfgs, guides (the guide list), start, goal)"""
    from edmp_amd.scenes import SyntheticDataset

    out = []
    for no, ncyl, (gl, bpg), scene_num, goal_idx in SPEC:
        ds = SyntheticDataset(scene_types=("stress",), num_scenes_per_type=3, n_obstacles=no, n_cylinders=ncyl)
        oc, _, _, ncub, nc, start, ik = ds.fetch_data(scene_num=scene_num, scene_type="stress")
        kinds = np.concatenate([np.zeros(int(ncub), dtype=np.int32), np.ones(int(nc), dtype=np.int32)])
        cfgs = cfgs_for(gl, bpg)
        assert cfgs["total_batch_size"] == B and oc.shape[0] == no and int(kinds.sum()) == ncyl
        out.append(dict(obstacle_config=oc, kinds=kinds, cfgs=cfgs, guides=list(gl), start=np.asarray(start, dtype=np.float64),
                        goal=np.asarray(ik[goal_idx], dtype=np.float64)))
    return out


def noises(draws=T + 1, seed=NOISE_SEED):
    """one (draws, B, 7, N) stream per scene"""
    rs = np.random.RandomState(seed)
    return [rs.standard_normal((draws, B, 7, N)) for _ in range(S)]


def random_state(parts, seed=5):
    """X (S, B, 7, N): every scene's joint-space line start -> goal plus white noise of amplitude 0 .. 0.3 rad, end columns pinned"""
    rs = np.random.RandomState(seed)
    t = np.linspace(0, 1, N)
    amp = np.linspace(0.0, 0.3, B)
    X = np.empty((len(parts), B, 7, N))
    for s, p in enumerate(parts):
        a, b = p["start"], p["goal"]
        X[s] = (a[:, None] * (1 - t) + b[:, None] * t)[None] + amp[:, None, None] * rs.standard_normal((B, 7, N))
        X[s, :, :, 0], X[s, :, :, -1] = a[None], b[None]
    return np.ascontiguousarray(X)
