#!/usr/bin/env python
"""batch_metrics_bench.py — what scoring a whole batch costs: evaluation.batch_metrics (edmp_metrics_rows_dev, csrc/metrics.hip)
against the single-trajectory host functions looped over the same rows.

    python scripts/batch_metrics_bench.py [--rows 1024] [--calls 200] [--warmup 20] [--out profiles/batch_metrics_bench.json]

Rows: the (1024, 7, 50) output of ONE real Diffusion.denoise_guided call - full-size TemporalUNet with seeded random weights, a
16-cuboid synthetic scene, guides [1, 2, 3, 4, 5, 10] dealt over the rows (the set-up of scripts/scene_batch_bench.py), z drawn on the
device.  Measured, each as a host clock around `calls` calls that ends in a synchronise, after `warmup` calls:
  (a) batch_metrics on the host array (upload + kernel + read-back of the four (B,) arrays),
  (b) batch_metrics on the device tensor with return_device=True (the kernel alone, as select_row uses it),
  (c) ONCE: the host loop path_lengths + smoothness_metric over the same rows on this box's CPU (one Python thread),
and the wall time of a second denoise_guided call of the same scene (device noise, result left on the device) to set them against.
Prints ONE JSON line and writes it to --out.  Informative: never bench.py's value."""
from __future__ import annotations

import argparse
import json
import os
import platform
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T, N, C = 255, 50, 7
DIMS = (32, 64, 128, 256, 512, 512)


def measure(rows=1024, guides=(1, 2, 3, 4, 5, 10), n_obstacles=16, calls=200, warmup=20, device="cuda:0", seed=0, commit=None):
    import torch

    from edmp_amd import evaluation as EV
    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.temporalunet import TemporalUNet

    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(n) for n in guides], rows // len(guides), T, rows_per_guide=GC.split_rows(rows, len(guides)))
    scene = scenes.random_scene(11, n_obstacles)
    guide = IntersectionVolumeGuide(scene, device, cfgs, rows)
    net = TemporalUNet(None, C, 32, device, dims=DIMS, state_dict=W.init_state_dict(5, C, 32, DIMS), max_batch=rows)
    dif = Diffusion(T, device)
    kw = dict(batch_size=rows, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL, noise="device", seed=seed, return_device=True)
    Xd = dif.denoise_guided(net, guide, N, C, cfgs["guidance_schedule"], **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Xd = dif.denoise_guided(net, guide, N, C, cfgs["guidance_schedule"], **kw)
    torch.cuda.synchronize()
    plan_s = time.perf_counter() - t0
    X = Xd.cpu().numpy()
    finite = np.isfinite(X).all(axis=(1, 2))

    def clock(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls

    host_in_s = clock(lambda: EV.batch_metrics(X, device=device))
    dev_in_s = clock(lambda: EV.batch_metrics(Xd, device=device, return_device=True))
    dev = EV.batch_metrics(Xd, device=device)
    t0 = time.perf_counter()
    host = np.full((4, rows), np.nan)
    for b in np.flatnonzero(finite):
        pl = EV.path_lengths(X[b])
        host[0, b], host[1, b] = pl["joint"], pl["end_effector"]
        host[2, b], host[3, b] = EV.smoothness_metric(X[b])
    host_loop_s = time.perf_counter() - t0
    err = max(float(np.max(np.abs(dev[k][finite] - host[i][finite]) / np.maximum(1.0, np.abs(host[i][finite])))) for i, k in enumerate(EV.METRIC_KEYS)) if finite.any() else None
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        pass
    return {
        "rows": rows, "N": N, "guides": list(guides), "obstacles": n_obstacles, "rows_finite": int(finite.sum()), "calls": calls, "warmup": warmup,
        "clock": "host perf_counter around `calls` calls ending in torch.cuda.synchronize(), after `warmup` calls; per call",
        "batch_metrics_host_input_s": host_in_s, "batch_metrics_device_input_return_device_s": dev_in_s,
        "host_loop_s": host_loop_s, "host_loop_is": "path_lengths + smoothness_metric per finite row, one Python thread, once, this box's CPU",
        "denoise_guided_s": plan_s, "denoise_guided_is": "second call of the same scene, device noise, result left on the device, wall clock ending in a synchronise",
        "host_loop_over_device_input": host_loop_s / dev_in_s, "host_loop_over_host_input": host_loop_s / host_in_s,
        "max_rel_error_vs_host_loop": err,
        "box": {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "torch": torch.__version__, "hip": torch.version.hip},
        "commit": commit, "commit_is": "the commit the measured working tree is based on",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "batch_metrics_bench.json"))
    ap.add_argument("--commit", type=str, default=None, help="commit the working tree is based on (default: git rev-parse, where the tree is a checkout)")
    a = ap.parse_args()
    if a.calls < 200 or a.warmup < 20:
        print("[batch_metrics_bench] fewer than 200 calls / 20 warm-up calls: a smoke run, not a measurement", file=sys.stderr)
    out = measure(a.rows, calls=a.calls, warmup=a.warmup, commit=a.commit)
    txt = json.dumps(out)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
