#!/usr/bin/env python
"""goal_filter_bench.py — what a group of k scenes costs between fetch_data and the first launch of the loop, two ways, in ONE process
on one GPU:

  per_scene  (infer_serial.prepare of the parent commit, unchanged by this work) per scene: IntersectionVolumeGuide(...) - it binds:
             edmp_scene_set, edmp_rows_set, the (B, T) schedule upload -, cost(goals, t = 0) + torch .sum + copy back + pick_goal;
             then SceneBatch(guides)
  batch      per scene IntersectionVolumeGuide(..., bind=False) - host tables only -, SceneBatch(guides), ONE SceneBatch.filter_goals
  filter     the filter_goals call of the batch route alone, on a batch that is already bound

    python scripts/goal_filter_bench.py [--ks 2,4,8] [--goals 100] [--rows 1024] [--reps 20] [--out profiles/goal_filter_bench.json]

Setting: the synthetic problem set of scene_batch_bench.py (16 obstacles of which 3 true cylinders, guides [1,2,3,4,5,10]), 100 IK goals
and B = 1024 rows per scene, k = 2, 4, 8.  Every repetition builds NEW guide objects, as the driver does for every group.  3 warm-up
repetitions, then --reps timed ones per route, interleaved; median and min-max of each.  Both routes pick the same goals (compared).
There is no gate on the ratio: the yardstick is the per_scene route of the same run.  Prints ONE JSON line.  Informative: never bench.py's
value."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def problems(k, n_goals, n_obstacles=16, n_cylinders=3):
    from edmp_amd.scenes import SyntheticDataset

    ds = SyntheticDataset("synthetic", scene_types=("tabletop", "stress"), num_scenes_per_type=(k + 1) // 2, n_obstacles=n_obstacles, n_cylinders=n_cylinders,
                          n_ik=n_goals)
    out = []
    for s in range(k):
        oc, _, _, ncub, nc, start, ik = ds.fetch_data(scene_num=s // 2, scene_type=("tabletop", "stress")[s % 2])
        out.append((oc, np.concatenate([np.zeros(int(ncub), dtype=np.int32), np.ones(int(nc), dtype=np.int32)]), np.asarray(start, dtype=np.float64), ik))
    return out


def spread(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "reps": int(a.size)}


def measure(ks=(2, 4, 8), n_goals=100, rows=1024, reps=20, warmup=3, device="cuda:0", guides=(1, 2, 3, 4, 5, 10)):
    import torch

    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch, pick_goal
    from edmp_amd.runtime import get_context

    ctx = get_context(device)
    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(n) for n in guides], rows // len(guides), 255, GC.split_rows(rows, len(guides)))
    out = {"rows_per_scene": rows, "goals_per_scene": n_goals, "obstacles": 16, "true_cylinders": 3, "guides": list(guides), "warmup": warmup,
           "clock": "host wall time around each route, the context synchronised before and after; routes interleaved repetition by repetition",
           "routes": {"per_scene": "k bound guide constructors + k cost filters + SceneBatch constructor (the parent commit's path)",
                      "batch": "k unbound guide constructors + SceneBatch constructor + one filter_goals",
                      "filter": "filter_goals alone on the bound batch"}}
    for k in ks:
        pr = problems(k, n_goals)
        starts = np.stack([p[2] for p in pr])

        def per_scene():
            gs, goals = [], []
            for oc, kinds, start, ik in pr:
                g = IntersectionVolumeGuide(oc, ctx, cfgs, rows, obstacle_kinds=kinds)
                volumes = g.cost(torch.tensor(ik.reshape((-1, 7, 1))), 0, batch_size=ik.shape[0]).sum(axis=(1, 2)).cpu().numpy()
                goals.append(pick_goal(volumes, ik, start)[1])
                gs.append(g)
            return SceneBatch(gs), np.stack(goals)

        def batched():
            b = SceneBatch([IntersectionVolumeGuide(oc, ctx, cfgs, rows, obstacle_kinds=kinds, bind=False) for oc, kinds, _, _ in pr])
            return b, b.filter_goals(starts, [p[3] for p in pr])[1]

        keep = {}

        def filter_only():
            return keep["batch"], keep["batch"].filter_goals(starts, [p[3] for p in pr])[1]

        times = {"per_scene": [], "batch": [], "filter": []}
        got = {}
        for rep in range(warmup + reps):
            for name, fn in (("per_scene", per_scene), ("batch", batched), ("filter", filter_only)):
                ctx.sync()
                t0 = time.perf_counter()
                b, goals = fn()
                ctx.sync()
                if rep >= warmup:
                    times[name].append(1e3 * (time.perf_counter() - t0))
                got[name] = goals
                if name == "batch":
                    keep["batch"] = b
        ps, bt = spread(times["per_scene"]), spread(times["batch"])
        out[f"k{k}"] = {"per_scene": ps, "batch": bt, "filter": spread(times["filter"]), "batch_over_per_scene_median": bt["median_ms"] / ps["median_ms"],
                        "goals_identical": bool(np.array_equal(got["per_scene"], got["batch"]) and np.array_equal(got["batch"], got["filter"]))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=str, default="2,4,8")
    ap.add_argument("--goals", type=int, default=100)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("at least 20 timed repetitions per route")
    out = measure(tuple(int(k) for k in a.ks.split(",")), a.goals, a.rows, a.reps)
    txt = json.dumps(out)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
