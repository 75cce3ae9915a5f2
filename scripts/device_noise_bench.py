#!/usr/bin/env python
"""device_noise_bench.py — what the noise source costs in the two run forms where the NumPy stream is a real cost, on ONE GPU:

  replan       Diffusion.denoise_guided(warm_start=WarmStart(best, t, renoise=True)) for t in --t-starts (16, 32, 64, 128) under three
               sources, interleaved repetition by repetition (scripts/replan_bench.py's method, 3 warm-up + --reps timed repetitions):
                 resident   a slice of one device tensor: no draw, no upload inside the clock (profiles/replan_bench.json's figure)
                 numpy      noise=None: the NumPy stream drawn (edmp_amd.nprng) and uploaded inside the clock
                 device     noise=DeviceNoise(seed): Philox inside the seed kernel and the step tail
  problem_set  infer_serial.run over --scenes (16) distinct scenes at k = 1, 2, 4 scenes per launch, with the feeder (NumPy stream) and
               with device_noise: wall time of the scene loop, mean noise_wait_s, steady-state scenes/s and the page-locked bytes the
               feeder holds (scripts/problem_set_bench.py's problem set and clock)

    python scripts/device_noise_bench.py [--rows 1024] [--reps 20] [--scenes 16] [--out profiles/device_noise_bench.json]

Setting: bench.py's flagship problem - the full-size net, B = 1024 rows, guides [1,2,3,4,5,10], 16 obstacles.  The weights are seeded, not
trained: only cost is measured.  Prints ONE JSON object.  Informative: never bench.py's value."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

from replan_bench import FULL_DIMS, C, N, T, spread  # noqa: E402


def replan(rows=1024, reps=20, warmup=3, t_starts=(16, 32, 64, 128), guides=(1, 2, 3, 4, 5, 10), n_obstacles=16, device="cuda:0"):
    import torch

    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd.diffusion import DeviceNoise, Diffusion, WarmStart
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import get_context
    from edmp_amd.temporalunet import TemporalUNet

    ctx = get_context(device)
    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(g) for g in guides], 0, T, rows_per_guide=GC.split_rows(rows, len(guides)))
    net = TemporalUNet(None, C, 32, ctx, dims=FULL_DIMS, seed=1, max_batch=rows)
    guide = IntersectionVolumeGuide(scenes.random_scene(11, n_obstacles), ctx, cfgs, rows)
    dif = Diffusion(T, ctx)
    start, goal = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    resident = ctx.to_dev(np.random.RandomState(1234).standard_normal((T + 1, rows, C, N)), torch.float64)
    kw = dict(batch_size=rows, start=start, goal=goal, return_device=True)
    X = dif.denoise_guided(net, guide, N, C, cfgs["guidance_schedule"], noise=resident, **kw)
    ctx.sync()
    best, _, _ = guide.select_row(start, goal, X)
    x0 = X[int(best)].clone()
    sources = {"resident": lambda t: resident[:1 + t], "numpy": lambda t: None, "device": lambda t: DeviceNoise(77)}
    routes = [(f"{src}_{t}", src, int(t)) for t in t_starts for src in sources]
    times = {name: [] for name, _, _ in routes}
    finite = {}
    np.random.seed(5)
    for rep in range(warmup + reps):
        for name, src, t in routes:
            ws = WarmStart(x0, t, renoise=True)
            ctx.sync()
            t0 = time.perf_counter()
            Y = dif.denoise_guided(net, guide, N, C, cfgs["guidance_schedule"], noise=sources[src](t), warm_start=ws, **kw)
            ctx.sync()
            if rep >= warmup:
                times[name].append(1e3 * (time.perf_counter() - t0))
            if rep == 0:
                finite[name] = bool(torch.isfinite(Y).all().item())
    out = {"rows": rows, "guides": list(guides), "obstacles": n_obstacles, "warmup": warmup,
           "clock": "host wall time around each denoise_guided call, the context synchronised before and after; routes interleaved repetition by repetition",
           "seed_plan": f"row {int(best)} of a full plan, given to all rows, renoise=True", "routes": {}}
    for name, src, t in routes:
        out["routes"][name] = dict(spread(times[name]), source=src, t_start=t, steps=t, finite=finite[name])
    for t in t_starts:
        base = out["routes"][f"resident_{t}"]["median_ms"]
        for src in ("numpy", "device"):
            out["routes"][f"{src}_{t}"]["over_resident_ms"] = out["routes"][f"{src}_{t}"]["median_ms"] - base
    return out


def problem_set(n_scenes=16, rows=1024, guides=(1, 2, 3, 4, 5, 10), n_obstacles=16, n_cylinders=3, groups=(1, 2, 4), device="cuda:0", seed=0):
    import torch
    import yaml

    import infer_serial
    from edmp_amd.runtime import get_context
    from edmp_amd.scenes import SyntheticDataset

    cfg = {
        "guide": {"guides": list(guides), "batch_size_per_guide": rows // len(guides), "total_rows": rows, "guide_path": "./guides/"},
        "dataset": {"path": "./datasets/", "dataset_type": "synthetic", "scene_types": ["tabletop", "stress"], "num_scenes_per_type": (n_scenes + 1) // 2},
        "model": {"model_dir": "./models/", "device": device, "T": T, "traj_len": N, "num_channels": C},
        "general": {"gui": False},
    }
    out = {"scenes": n_scenes, "rows_per_scene": rows, "groups": list(groups),
           "clock": "wall time of infer_serial.run's scene loop (the run's model build / upload excluded); steady_state = between the end of the first group "
                    "and the end of the last; pinned_bytes = the page-locked whole-scene buffers the feeder holds for the run (0 with device_noise)"}
    base = get_context(device)
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(os.path.join(td, "configs"))
        path = os.path.join(td, "configs", "cfg_problem_set.yaml")
        with open(path, "w") as f:
            yaml.safe_dump(cfg, f)
        ds = SyntheticDataset("synthetic", scene_types=("tabletop", "stress"), num_scenes_per_type=(n_scenes + 1) // 2, n_obstacles=n_obstacles, n_cylinders=n_cylinders)

        def leg(k, dn):
            np.random.seed(seed)
            infer_serial.run(path, dataset=ds, max_scenes=k, verbose=False, scenes_per_launch=k, shard_scenes=False, device_noise=dn)  # untimed: upload, kernel attributes
            np.random.seed(seed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = infer_serial.run(path, dataset=ds, max_scenes=n_scenes, verbose=False, scenes_per_launch=k, shard_scenes=False, device_noise=dn)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0 - infer_serial.run.last_setup_s
            done = [r["done_at"] for r in res]
            steady = (n_scenes - k) / (done[-1] - done[k - 1]) if n_scenes > k else n_scenes / wall
            bufs = getattr(base, "_scene_noise_buffers", None) or []
            return {
                "wall_s": wall, "scenes_per_s": n_scenes / wall, "steady_state_scenes_per_s": steady,
                "noise_wait_s_mean": float(np.mean([r["timings"].get("noise_wait_s", 0.0) for r in res])),
                "denoise_s_mean": float(np.mean([r["timings"]["denoise_s"] for r in res])),
                "pinned_bytes": int(sum(b.numel() * b.element_size() for b in bufs)),
            }

        for k in groups:
            for source in ("feeder", "device_noise"):
                dn = 11 if source == "device_noise" else None
                base._scene_noise_buffers = None  # (the feeder's cache: each leg holds what it allocates itself)
                try:
                    out[f"k{k}_{source}"] = leg(k, dn)
                except Exception as exc:  # (e.g. the feeder's page-locked allocation: 2k x 734 MB at 1024 rows)
                    out[f"k{k}_{source}"] = {"error": f"{type(exc).__name__}: {exc}"}
        base._scene_noise_buffers = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--t-starts", type=str, default="16,32,64,128")
    ap.add_argument("--groups", type=str, default="1,2,4")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("at least 20 timed repetitions per route")
    out = {"what": "noise sources of warm starts and scene groups: resident tensor / NumPy stream / device source (Philox)",
           "replan": replan(a.rows, a.reps, t_starts=tuple(int(t) for t in a.t_starts.split(","))),
           "problem_set": problem_set(a.scenes, a.rows, groups=tuple(int(k) for k in a.groups.split(",")))}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
