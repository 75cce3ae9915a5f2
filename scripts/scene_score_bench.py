#!/usr/bin/env python
"""scene_score_bench.py — what scoring one finished group of k scenes costs, two ways, in ONE process on one GPU:

  per_scene  host X (k, B, 7, N); for every scene its own guide: select_row (upload of X[s], swept volumes, arg-min) and success_rows
             (second upload of X[s], success kernel, counts) - what infer_serial.plan_group did before the batch could score itself
  batch      device X; SceneBatch.select_rows + SceneBatch.success_rows: one swept-volume launch, one segmented arg-min, one success launch,
             one count launch for the whole group

    python scripts/scene_score_bench.py [--ks 2,4,8] [--rows 1024] [--reps 20] [--driver-before PATH] [--out profiles/scene_score_bench.json]

Setting: the synthetic problem set of scene_batch_bench.py (16 obstacles of which 3 true cylinders, guides [1,2,3,4,5,10]), B = 1024 rows per
scene, k = 2, 4, 8.  X is built by hand - every scene's joint-space line start -> goal plus white noise at amplitudes from 0 to 3 rad, so
that rows leave the joint limits in a mix - and both routes score the same X (their answers are compared).  Two placements of the obstacles,
because the success kernel leaves a row at its first hit: `as_placed` (in these synthetic scenes every row touches an obstacle: the kernel's
cheap case) and `scene_10m_away` (every obstacle moved 10 m along x: no row collides, every configuration x link x obstacle is tested: its
dear case).  3 warm-up repetitions, then --reps timed ones per route, interleaved; median and min-max of each.  The yardstick is the
per_scene route of the same run.  `x_to_host_ms` (what bringing the state back once costs) is reported beside them: the per_scene route has
paid it before it starts, the batch route pays it after scoring, for the result dicts.

--driver-before PATH: also the group wall time of infer_serial.run at k = 4 (scripts/scene_batch_bench.py's measure) with the driver in PATH
(the parent commit's infer_serial.py: `git show HEAD~1:infer_serial.py > PATH`) and with this tree's, into the same JSON.
Prints ONE JSON line.  Informative: never bench.py's value."""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

N = 50
AMPS = (0.0, 1e-3, 0.01, 0.03, 0.1, 0.3, 1.0, 3.0)


def group(k, rows, device, shift=0.0, guides=(1, 2, 3, 4, 5, 10), n_obstacles=16, n_cylinders=3, seed=0):
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.scenes import SyntheticDataset

    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(n) for n in guides], rows // len(guides), 255, GC.split_rows(rows, len(guides)))
    ds = SyntheticDataset("synthetic", scene_types=("tabletop", "stress"), num_scenes_per_type=(k + 1) // 2, n_obstacles=n_obstacles, n_cylinders=n_cylinders)
    rs = np.random.RandomState(seed)
    t = np.linspace(0, 1, N)
    gs, starts, goals, X = [], [], [], np.empty((k, rows, 7, N))
    for s in range(k):
        oc, _, _, ncub, nc, start, ik = ds.fetch_data(scene_num=s // 2, scene_type=("tabletop", "stress")[s % 2])
        kinds = np.concatenate([np.zeros(int(ncub), dtype=np.int32), np.ones(int(nc), dtype=np.int32)])
        oc = oc.copy()
        oc[:, 0] += shift
        gs.append(IntersectionVolumeGuide(oc, device, cfgs, rows, obstacle_kinds=kinds))
        starts.append(start)
        goals.append(ik[0])
        amp = rs.choice(AMPS, size=rows)
        X[s] = (start[:, None] * (1 - t) + ik[0][:, None] * t)[None] + amp[:, None, None] * rs.standard_normal((rows, 7, N))
        X[s, :, :, 0], X[s, :, :, -1] = start[None], ik[0][None]
    return gs, np.stack(starts), np.stack(goals), X


def spread(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "reps": int(a.size)}


def measure(ks=(2, 4, 8), rows=1024, reps=20, warmup=3, device="cuda:0"):
    import torch

    from edmp_amd.guide import SceneBatch
    from edmp_amd.runtime import get_context

    ctx = get_context(device)
    out = {"rows_per_scene": rows, "waypoints": N, "obstacles": 16, "true_cylinders": 3, "guides": [1, 2, 3, 4, 5, 10], "warmup": warmup,
           "state": f"hand-built: line start -> goal + a * N(0, 1), a drawn per row from {list(AMPS)}, start / goal columns pinned",
           "clock": "host wall time around each route, the context synchronised before and after; routes interleaved repetition by repetition",
           "acceptance": "batch median <= per_scene median + (per_scene max - per_scene min)"}
    for placement, shift, k in [(p, sh, k) for p, sh in (("as_placed", 0.0), ("scene_10m_away", 10.0)) for k in ks]:
        gs, starts, goals, X = group(k, rows, ctx, shift)
        batch = SceneBatch(gs)
        Xd = ctx.to_dev(X, torch.float64)
        ctx.sync()

        def per_scene():
            res = []
            for s, g in enumerate(gs):
                idx, vols, _ = g.select_row(starts[s], goals[s], X[s])
                res.append((idx, vols, g.success_rows(X[s])))
            return res

        def batched():
            idx, vols, _ = batch.select_rows(starts, goals, Xd)
            return idx, vols, batch.success_rows(Xd)

        times = {"per_scene": [], "batch": [], "x_to_host": []}
        for rep in range(warmup + reps):
            for name, fn in (("per_scene", per_scene), ("batch", batched), ("x_to_host", lambda: ctx.to_host(Xd))):
                ctx.sync()
                t0 = time.perf_counter()
                r = fn()
                ctx.sync()
                if rep >= warmup:
                    times[name].append(1e3 * (time.perf_counter() - t0))
                if name == "per_scene":
                    ref = r
                elif name == "batch":
                    got = r
        same = all(int(got[0][s]) == ref[s][0] and np.array_equal(got[1][s], ref[s][1], equal_nan=True) and
                   all(np.array_equal(got[2][key][s], ref[s][2][key]) for key in ("ok", "first", "within")) and
                   int(got[2]["rows_ok"][s]) == ref[s][2]["rows_ok"] for s in range(k))
        ps, bt = spread(times["per_scene"]), spread(times["batch"])
        out.setdefault(placement, {})[f"k{k}"] = {"per_scene": ps, "batch": bt, "x_to_host_ms": spread(times["x_to_host"]), "batch_over_per_scene_median": bt["median_ms"] / ps["median_ms"],
                        "accepted": bool(bt["median_ms"] <= ps["median_ms"] + (ps["max_ms"] - ps["min_ms"])), "answers_identical": bool(same),
                        "rows_collision_free_per_scene": [int(v) for v in got[2]["rows_collision_free"]], "rows_within_per_scene": [int(v) for v in got[2]["rows_within"]]}
    return out


def driver_group_wall(before_path, scenes=8, k=4):
    """infer_serial.run's wall time per group at k scenes per launch, with the driver module in `before_path` and with this tree's"""
    import scene_batch_bench as SBB

    out = {"scenes": scenes, "k": k, "source": "scripts/scene_batch_bench.py measure(): wall_s / groups, planning_time_s_mean"}
    mods = {"after": os.path.join(ROOT, "infer_serial.py"), "before": before_path}
    for name in ("before", "after", "before_again", "after_again"):  # (twice each, alternating: the spread between equal runs is the noise)
        spec = importlib.util.spec_from_file_location("infer_serial", mods[name.split("_")[0]])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["infer_serial"] = mod
        spec.loader.exec_module(mod)
        r = SBB.measure(n_scenes=scenes, ks=(k,))[f"k{k}"]
        groups = (scenes + k - 1) // k
        out[name] = {"group_wall_s": r["wall_s"] / groups, "denoise_s_mean_per_group": r["denoise_s_mean_per_group"], "planning_time_s_mean": r["planning_time_s_mean"],
                     "traj_steps_per_s": r["traj_steps_per_s"]}
    sys.modules.pop("infer_serial", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=str, default="2,4,8")
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--driver-before", type=str, default=None, help="the parent commit's infer_serial.py: also measure the k = 4 group wall time before / after")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("at least 20 timed repetitions per route")
    out = measure(tuple(int(k) for k in a.ks.split(",")), a.rows, a.reps)
    if a.driver_before:
        out["infer_serial_k4"] = driver_group_wall(a.driver_before)
    txt = json.dumps(out)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
