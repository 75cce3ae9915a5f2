#!/usr/bin/env python
"""ik_bench.py — what the IK goal candidates of a scene group cost on the GPU, in ONE process on one GPU:

  solve       ik.solve(targets, seeds, return_device=True): seed upload, edmp_ik_solve_dev, edmp_ik_compact_dev, the counts back on the host
  to_goals    the same call, then SceneBatch.filter_goals(starts, goals_dev, counts=...) on a bound batch: from target poses to one picked
              goal per scene, the candidates never leaving the device
  host        the NumPy restatement of the same iteration (tests/ik_inputs.dls_numpy), target after target, on this box's CPU - context
              only: it is the tests' reference, not a product path (the package has no host solver)

    python scripts/ik_bench.py [--ts 1,4,8] [--seeds 256] [--iters 64] [--reps 20] [--out profiles/ik_bench.json]

Setting: the tests' fixed inputs (tests/ik_inputs.py: 8 target poses = FK of configurations inside the middle 70 % of the joint ranges, 256
uniform seeds per target), the first T of them; scenes of 16 obstacles (3 true cylinders), 1024 rows per scene as in goal_filter_bench.py.
3 warm-up repetitions, then --reps timed ones per route, interleaved; median and min-max of each; the context synchronised before and
after.  Also records the per-target yields of the GPU and of the restatement.  No gate.  Prints ONE JSON line.  Informative: never bench.py's
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


def spread(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "reps": int(a.size)}


def scene_batch(k, rows, ctx, guides=(1, 2, 3, 4, 5, 10)):
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch
    from edmp_amd.scenes import SyntheticDataset

    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(n) for n in guides], rows // len(guides), 255, GC.split_rows(rows, len(guides)))
    ds = SyntheticDataset("synthetic", scene_types=("tabletop", "stress"), num_scenes_per_type=(k + 1) // 2, n_obstacles=16, n_cylinders=3, n_ik=1)
    gs, starts = [], []
    for s in range(k):
        oc, _, _, ncub, nc, start, _ = ds.fetch_data(scene_num=s // 2, scene_type=("tabletop", "stress")[s % 2])
        kinds = np.concatenate([np.zeros(int(ncub), dtype=np.int32), np.ones(int(nc), dtype=np.int32)])
        gs.append(IntersectionVolumeGuide(oc, ctx, cfgs, rows, obstacle_kinds=kinds, bind=False))
        starts.append(np.asarray(start, dtype=np.float64))
    return SceneBatch(gs), np.stack(starts)


def measure(ts=(1, 4, 8), n_seeds=256, iters=64, rows=1024, reps=20, warmup=3, device="cuda:0"):
    from edmp_amd import ik
    from edmp_amd.runtime import get_context
    from tests import ik_inputs as I

    ctx = get_context(device)
    out = {"seeds_per_target": n_seeds, "iters": iters, "damping": ik.DAMPING, "max_step": ik.MAX_STEP, "tol_pos": ik.TOL_POS, "tol_ang": ik.TOL_ANG,
           "rows_per_scene": rows, "obstacles": 16, "warmup": warmup,
           "clock": "host wall time around each route, the context synchronised before and after; routes interleaved repetition by repetition",
           "routes": {"solve": "ik.solve(..., return_device=True): upload, solve kernel, compaction, counts on the host",
                      "to_goals": "solve + SceneBatch.filter_goals on the device goals (bound batch): target poses -> one picked goal per scene",
                      "host": "tests/ik_inputs.dls_numpy per target on the CPU (the tests' reference; context only)"}}
    for T in ts:
        targets = I.targets()[:T]
        seeds = [s[:n_seeds] for s in I.seeds()[:T]]
        batch, starts = scene_batch(T, rows, ctx)
        first = ik.solve(ctx, targets, seeds, iters=iters, return_device=True)
        batch.filter_goals(starts, first["goals"], counts=first["counts"])  # binds the batch

        def solve_only():
            return ik.solve(ctx, targets, seeds, iters=iters, return_device=True)

        def to_goals():
            r = ik.solve(ctx, targets, seeds, iters=iters, return_device=True)
            return batch.filter_goals(starts, r["goals"], counts=r["counts"])

        def host():
            return [I.dls_numpy(tg, sd, iters=iters) for tg, sd in zip(targets, seeds)]

        times = {"solve": [], "to_goals": [], "host": []}
        got = {}
        for rep in range(warmup + reps):
            for name, fn in (("solve", solve_only), ("to_goals", to_goals), ("host", host)):
                if name == "host" and rep >= warmup + 5:
                    continue  # (tens of milliseconds each and steady: five repetitions)
                ctx.sync()
                t0 = time.perf_counter()
                got[name] = fn()
                ctx.sync()
                if rep >= warmup:
                    times[name].append(1e3 * (time.perf_counter() - t0))
        out[f"T{T}"] = {"solve": spread(times["solve"]), "to_goals": spread(times["to_goals"]), "host": spread(times["host"]),
                        "valid_per_target_gpu": [int(c) for c in got["solve"]["counts"]], "valid_per_target_host": [int(v.sum()) for _, _, v in got["host"]],
                        "picked_index_per_scene": [int(i) for i in got["to_goals"][0]]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", type=str, default="1,4,8")
    ap.add_argument("--seeds", type=int, default=256)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("at least 20 timed repetitions per route")
    out = measure(tuple(int(t) for t in a.ts.split(",")), a.seeds, a.iters, a.rows, a.reps)
    txt = json.dumps(out)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
