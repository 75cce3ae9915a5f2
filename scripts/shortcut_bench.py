#!/usr/bin/env python
"""shortcut_bench.py — what the shortcut stage (shortcut_rows_kernel, csrc/shortcut.hip) costs: edmp_shortcut_rows_dev on a device state of
1024 x (7, 50) rows among 16 obstacles at substeps K = 4 with passes = 1, 2 and 4.  The rows are the straight line from start to goal with a
half-sine bump of a random height per row and joint and a zigzag on top, so that spans are tested, accepted and rejected.

    python scripts/shortcut_bench.py [--rows 1024] [--calls 20] [--warmup 3] [--out profiles/shortcut_bench.json]

A sample is one call on a fresh device copy of the state (the copy is made and synchronised outside the timed window; the entry point
itself ends in a stream synchronise), timed by a host clock; each figure is the median of `calls` samples after `warmup`, the three pass
counts taken alternately.  The mean number of tested candidates and accepted spans per row is recorded beside each time.

With --self-safe-out FILE the script runs ONE other leg instead: guide.shortcut_rows on the same state at passes = 2 with self_pairs=None
and self_pairs=True (the self-collision test of the candidates, shortcut_rows_kernel<true>), the two taken alternately, medians of `calls`
calls each inside a host window closed by the context's synchronise, with the rejected counts; the record goes under "shortcut" into FILE
(profiles/self_safe_bench.json, which scripts/blend_bench.py shares).

Prints ONE JSON line and writes it to --out.  Informative: no time is gated, and this is never bench.py's value."""
from __future__ import annotations

import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T, N, K = 255, 50, 4
PASSES = (1, 2, 4)
MIN_GAIN = 1e-6
# scenes.random_scene(12, 16) with every extent x 0.35: start and goal are free, the straight line collides, and the rows below see both
# accepted and rejected candidates (searched on the CPU with the success check's host twin; random_scene's own boxes leave no row free)
SCENE_SEED, SCENE_SCALE = 12, 0.35


def measure(rows=1024, calls=20, warmup=3, device="cuda:0", commit=None):
    import torch

    from edmp_amd import _capi, franka, scenes
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import ptr

    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(1)], rows, T)
    scene = scenes.random_scene(SCENE_SEED, 16)
    scene[:, 7:10] *= SCENE_SCALE
    guide = IntersectionVolumeGuide(scene, device, cfgs, rows)
    guide._bind()
    ctx = guide.ctx
    s, g = np.ascontiguousarray(scenes.DEFAULT_START, dtype=np.float64), np.ascontiguousarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    f = np.linspace(0, 1, N)
    rs = np.random.RandomState(3)
    X = s[None, :, None] * (1 - f) + g[None, :, None] * f + rs.uniform(-0.6, 0.6, size=(rows, 7, 1)) * np.sin(np.pi * f)[None, None, :]
    X[:, 3, 1:-1] += 0.1 * (-1.0) ** np.arange(1, N - 1)
    X[:, :, 0], X[:, :, -1] = s, g
    X0 = ctx.to_dev(np.ascontiguousarray(X), torch.float64)
    counts, length = ctx.empty((2, rows), torch.int32), ctx.empty((rows, 2), torch.float64)
    dh = np.ascontiguousarray(franka.dh_table_f64())

    def sample(passes):
        with torch.cuda.stream(ctx.stream):
            Xw = X0.clone()
        ctx.sync()
        t0 = time.perf_counter()
        _capi.check(ctx.lib.edmp_shortcut_rows_dev(ctx.h, ptr(Xw), rows, N, None, 0, K, passes, MIN_GAIN, _capi.as_pd(dh), ptr(counts[0]), ptr(counts[1]), ptr(length),
                                                   None, 0), "edmp_shortcut_rows_dev")
        dt = time.perf_counter() - t0
        return dt, ctx.to_host(counts), ctx.to_host(length)

    times = {n: [] for n in PASSES}
    work = {}
    for k in range(warmup + calls):
        for n in PASSES:  # alternating: all see the same box at the same time
            dt, c, ln = sample(n)
            work[n] = dict(tested_per_row=float(c[1].mean()), accepted_per_row=float(c[0].mean()), rows_shortened=int((c[0] > 0).sum()),
                           mean_length_before=float(ln[:, 0].mean()), mean_length_after=float(ln[:, 1].mean()))
            if k >= warmup:
                times[n].append(dt)
    before = guide.success_rows(X0)["rows_collision_free"]
    after = guide.success_rows(guide.shortcut_rows(X0, passes=PASSES[-1], substeps=K, log_cap=0, return_device=True)["trajectories"])["rows_collision_free"]
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        pass
    med = {n: statistics.median(v) for n, v in times.items()}
    return {
        "rows": rows, "N": N, "obstacles": 16, "scene": f"scenes.random_scene({SCENE_SEED}, 16), extents x {SCENE_SCALE}", "substeps": K, "min_gain": MIN_GAIN, "calls": calls, "warmup": warmup,
        "clock": "median of `calls` samples per pass count, taken alternately; a sample is ONE edmp_shortcut_rows_dev call (it ends in a stream synchronise) on a "
                 "fresh device copy of the state inside a host perf_counter window",
        "call_s": {f"passes{n}": med[n] for n in PASSES},
        "spread_s": {f"passes{n}": [min(v), max(v)] for n, v in times.items()},
        "work": {f"passes{n}": work[n] for n in PASSES},
        "call_over_tested_candidates_per_row_s": {f"passes{n}": med[n] / max(work[n]["tested_per_row"], 1e-9) for n in PASSES},
        "rows_collision_free_before": int(before), "rows_collision_free_after_passes4": int(after),
        "box": {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "torch": torch.__version__, "hip": torch.version.hip},
        "commit": commit, "commit_is": "the commit the measured working tree is based on",
    }


def merge_into(path, key, record):
    """put `record` under `key` into the JSON object in `path` (made if absent)"""
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[key] = record
    with open(path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def bench_state(rows, device="cuda:0"):
    """the guide and the device state of this script's scene and rows (measure builds the same)"""
    import torch

    from edmp_amd import scenes
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(1)], rows, T)
    scene = scenes.random_scene(SCENE_SEED, 16)
    scene[:, 7:10] *= SCENE_SCALE
    guide = IntersectionVolumeGuide(scene, device, cfgs, rows)
    s, g = np.ascontiguousarray(scenes.DEFAULT_START, dtype=np.float64), np.ascontiguousarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    f = np.linspace(0, 1, N)
    rs = np.random.RandomState(3)
    X = s[None, :, None] * (1 - f) + g[None, :, None] * f + rs.uniform(-0.6, 0.6, size=(rows, 7, 1)) * np.sin(np.pi * f)[None, None, :]
    X[:, 3, 1:-1] += 0.1 * (-1.0) ** np.arange(1, N - 1)
    X[:, :, 0], X[:, :, -1] = s, g
    return guide, guide.ctx.to_dev(np.ascontiguousarray(X), torch.float64)


def alternate(ctx, call, calls, warmup):
    """call(self_pairs) with self_pairs = None ("off") and True ("on") taken alternately, each inside a host window closed by the context's
    synchronise -> (medians, [min, max], the last result of each leg)"""
    legs = {"off": None, "on": True}
    times, last = {k: [] for k in legs}, {}
    for k in range(warmup + calls):
        for name, pairs in legs.items():  # alternating: both see the same box at the same time
            ctx.sync()
            t0 = time.perf_counter()
            last[name] = call(pairs)
            ctx.sync()
            if k >= warmup:
                times[name].append(time.perf_counter() - t0)
    return {k: statistics.median(v) for k, v in times.items()}, {k: [min(v), max(v)] for k, v in times.items()}, last


def measure_self_safe(rows=1024, calls=20, warmup=3, passes=2):
    """the self-safe leg: the same state and scene, guide.shortcut_rows with self_pairs=None and True"""
    import torch

    guide, X0 = bench_state(rows)
    med, spread, last = alternate(guide.ctx, lambda pairs: guide.shortcut_rows(X0, passes=passes, substeps=K, log_cap=0, return_device=True, self_pairs=pairs), calls, warmup)
    free = lambda X: int(guide.self_collision_rows(X, substeps=K)["free"].sum())  # noqa: E731
    return {
        "rows": rows, "N": N, "obstacles": 16, "substeps": K, "passes": passes, "calls": calls, "warmup": warmup, "pair_mask": "franka.self_collision_pairs(): 18 pairs, 6 lower links",
        "clock": "median of `calls` guide.shortcut_rows(return_device=True) calls per leg, taken alternately, each with the context's synchronise inside a host perf_counter window",
        "call_s": med, "spread_s": spread, "on_over_off": med["on"] / med["off"],
        "tested_per_row": {k: float(v["tested"].float().mean()) for k, v in last.items()}, "accepted_per_row": {k: float(v["accepted"].float().mean()) for k, v in last.items()},
        "self_rejected": int(last["on"]["self_rejected"].sum()), "rows_with_a_self_rejection": int((last["on"]["self_rejected"] > 0).sum()),
        "rows_self_collision_free_before": free(X0), "rows_self_collision_free_after": {k: free(v["trajectories"]) for k, v in last.items()},
        "box": {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "torch": torch.__version__, "hip": torch.version.hip},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "shortcut_bench.json"))
    ap.add_argument("--commit", type=str, default=None, help="commit the working tree is based on (default: git rev-parse, where the tree is a checkout)")
    ap.add_argument("--self-safe-out", type=str, default=None, help="run the self-safe leg alone and put its record under \"shortcut\" into this JSON file")
    a = ap.parse_args()
    if a.self_safe_out:
        out = measure_self_safe(a.rows, calls=a.calls, warmup=a.warmup)
        print(json.dumps(out))
        merge_into(a.self_safe_out, "shortcut", out)
        return
    out = measure(a.rows, calls=a.calls, warmup=a.warmup, commit=a.commit)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
