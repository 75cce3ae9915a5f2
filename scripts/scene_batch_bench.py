#!/usr/bin/env python
"""scene_batch_bench.py — the problem set of problem_set_bench.py (16 distinct synthetic scenes, 1024 rows, guides [1,2,3,4,5,10],
16 obstacles of which 3 true cylinders, noise from NumPy's global RandomState per scene) planned k scenes per launch chain
(infer_serial.run(scenes_per_launch=k): Diffusion.denoise_guided_scenes over a guide.SceneBatch), k = 1, 2, 4 in ONE process.

    python scripts/scene_batch_bench.py [--scenes 16] [--ks 1,2,4] [--out PATH]

Prints ONE JSON line: per k the wall and steady-state traj-steps/s and the mean noise_wait_s (time the group waited for the feeder's
whole-scene streams - when the host draw, ~0.6 ms per 1024-row step, is the ceiling, it shows here), and the ratios against k = 1.
Every k plans the same scenes under the same seed, so their results are also checked to be identical.  Informative: never bench.py's value."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import yaml  # noqa: E402

T, N, C = 255, 50, 7


def measure(n_scenes=16, rows=1024, guides=(1, 2, 3, 4, 5, 10), n_obstacles=16, n_cylinders=3, ks=(1, 2, 4), device="cuda:0", seed=0):
    import torch

    import infer_serial
    from edmp_amd.scenes import SyntheticDataset

    cfg = {
        "guide": {"guides": list(guides), "batch_size_per_guide": rows // len(guides), "total_rows": rows, "guide_path": "./guides/"},
        "dataset": {"path": "./datasets/", "dataset_type": "synthetic", "scene_types": ["tabletop", "stress"], "num_scenes_per_type": (n_scenes + 1) // 2},
        "model": {"model_dir": "./models/", "device": device, "T": T, "traj_len": N, "num_channels": C},
        "general": {"gui": False},
    }
    out = {"scenes": n_scenes, "rows_per_scene": rows, "guides": list(guides), "obstacles": n_obstacles, "true_cylinders": n_cylinders,
           "noise": "NumPy global RandomState per scene, in scene order (the reference's contract)",
           "clock": "wall time of infer_serial.run's scene loop (model build / upload excluded); steady state = between the end of the first group of k scenes "
                    "and the end of the last (n - k scenes)"}
    trajectories = {}
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(os.path.join(td, "configs"))
        path = os.path.join(td, "configs", "cfg_scene_batch.yaml")
        with open(path, "w") as f:
            yaml.safe_dump(cfg, f)
        ds = SyntheticDataset("synthetic", scene_types=("tabletop", "stress"), num_scenes_per_type=(n_scenes + 1) // 2, n_obstacles=n_obstacles, n_cylinders=n_cylinders)
        for k in ks:  # one untimed group per k: model build, pinned feeder buffers, kernel attributes
            np.random.seed(seed)
            infer_serial.run(path, dataset=ds, max_scenes=k, verbose=False, shard_scenes=False, scenes_per_launch=k)
        for k in ks:
            np.random.seed(seed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = infer_serial.run(path, dataset=ds, max_scenes=n_scenes, verbose=False, shard_scenes=False, scenes_per_launch=k)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0 - infer_serial.run.last_setup_s
            assert len(res) == n_scenes
            done = [r["done_at"] for r in res]
            steady = (n_scenes - k) / (done[-1] - done[k - 1]) if n_scenes > k else n_scenes / wall
            n_groups = (n_scenes + k - 1) // k
            # noise_wait_s / denoise_s are per group (every scene of a group carries its group's value)
            firsts = [res[g * k] for g in range(n_groups)]
            out[f"k{k}"] = {
                "wall_s": wall, "traj_steps_per_s": n_scenes * rows * T / wall, "steady_state_traj_steps_per_s": steady * rows * T,
                "noise_wait_s_mean_per_group": float(np.mean([r["timings"].get("noise_wait_s", 0.0) for r in firsts])),
                "denoise_s_mean_per_group": float(np.mean([r["timings"]["denoise_s"] for r in firsts])),
                "planning_time_s_mean": float(np.mean([r["planning_time_s"] for r in res])),
                "success_proxy_collision_free": int(sum(r["success_proxy"] for r in res)),
            }
            trajectories[k] = [r["trajectory"] for r in res]
    base = out[f"k{ks[0]}"]
    for k in ks[1:]:
        o = out[f"k{k}"]
        o["x_vs_k1"] = o["traj_steps_per_s"] / base["traj_steps_per_s"]
        o["steady_x_vs_k1"] = o["steady_state_traj_steps_per_s"] / base["steady_state_traj_steps_per_s"]
        o["identical_to_k1"] = all(np.array_equal(a, b) for a, b in zip(trajectories[ks[0]], trajectories[k]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--ks", type=str, default="1,2,4", help="scenes per launch to measure")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    out = measure(a.scenes, a.rows, ks=tuple(int(k) for k in a.ks.split(",")))
    txt = json.dumps(out)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
