#!/usr/bin/env python
"""sdf_guide_bench.py — what the sphere signed-distance guide (edmp_amd/csrc/sdf.hip) costs on one GPU, B = 1024, full TemporalUNet,
noise resident on the device.  No gate: nothing here had been timed before.

    python scripts/sdf_guide_bench.py [--reps 20] [--parent-root DIR] [--only group] [--out profiles/sdf_guide_bench.json]

  flagship        a full plan (denoise_guided, 255 steps) with the six-guide ensemble [1,2,3,4,5,10] on a 16-obstacle scene - no SDF rows, so
                  the launches are those of the parent commit.  With --parent-root DIR (a built checkout of the parent commit) the same plan
                  is timed there too, each tree in child processes of its own, alternating parent / this / parent / this: the two must agree
                  within the spread the file records.
  sdf_plan        the same plan with guide 10 replaced by the SDF guide 101 (171 SDF rows, default spheres), on the 16-obstacle scene and on
                  a 64-obstacle scene, beside the six-guide plan on the same scene in the same process.
  kernel          sdf_guide_kernel in the stream: edmp_guide_gradient_dev on device tensors, enqueued back to back between two events, with
                  k SDF rows minus the same call with none (k = 171 and 1024; 16 and 64 obstacles).  The volume kernel of the same call
                  (guide_kernel, 28 us per launch in DESIGN.md) runs in both.
  group           four 16-obstacle scenes planned with the ensemble [1,2,3,4,5,101] (171 SDF rows per scene) one scene per launch chain
                  (k = 1: four denoise_guided calls, one guide per scene) and as one scene group (k = 4: one denoise_guided_scenes call on a
                  guide.SceneBatch, 4096 rows), the same resident noise in both; the time is that of the four scenes.  --only group runs this
                  leg alone.

Medians of --reps calls after 3 warm-up calls, with min / max.  Clock: host wall time around a synchronised call for the plans, HIP events on
the context's stream for the kernel.  Prints ONE JSON line.  Informative: never bench.py's value."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, C, B = 255, 50, 7, 1024
FLAGSHIP = (1, 2, 3, 4, 5, 10)
WARMUP = 3


def spread(ms):
    import numpy as np

    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "reps": int(a.size)}


def setup(device="cuda:0"):
    import numpy as np
    import torch

    from edmp_amd.diffusion import Diffusion
    from edmp_amd.temporalunet import TemporalUNet

    net = TemporalUNet(None, C, 32, device, dims=(32, 64, 128, 256, 512, 512), seed=1, max_batch=B)
    dif = Diffusion(T, device)
    ctx = dif.ctx
    noise = ctx.to_dev(np.random.RandomState(1234).standard_normal((T + 1, B, C, N)), torch.float64)
    ctx.sync()
    return net, dif, ctx, noise


def plan_times(net, dif, ctx, noise, guides, n_obstacles, reps):
    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = GC.build_guide_cfgs([GC.load_guide_dict(g) for g in guides], 0, T, rows_per_guide=GC.split_rows(B, len(guides)))
    guide = IntersectionVolumeGuide(scenes.random_scene(11, n_obstacles), ctx, cfgs, B)
    start, goal = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    ms = []
    for rep in range(WARMUP + reps):
        ctx.sync()
        t0 = time.perf_counter()
        dif.denoise_guided(net, guide, N, C, cfgs["guidance_schedule"], batch_size=B, start=start, goal=goal, noise=noise, return_device=True)
        ctx.sync()
        if rep >= WARMUP:
            ms.append(1e3 * (time.perf_counter() - t0))
    out = spread(ms)
    out["sdf_rows"] = int(cfgs["sdf_rows"].sum()) if "sdf_rows" in cfgs else 0
    return out


def kernel_times(ctx, reps, calls=50):
    """per-call stream time of edmp_guide_gradient_dev with k SDF rows and with none, on the same scene, rows and joints"""
    import numpy as np
    import torch

    from edmp_amd import _capi, franka, scenes
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import ptr

    out = {}
    lo, hi = franka.joint_limits()
    q = ctx.to_dev(np.random.RandomState(5).uniform(lo[None, :, None], hi[None, :, None], (B, C, N - 2)), torch.float64)
    grad = ctx.empty((B, C, N - 2), torch.float64)
    start, goal = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    for n_obstacles in (16, 64):
        scene = scenes.random_scene(11, n_obstacles)
        per = {}
        for k in (0, 171, 1024):
            cfgs = GC.build_guide_cfgs([GC.load_guide_dict(g) for g in (1, 101)], 0, T, rows_per_guide=[B - k, k]) if k else \
                GC.build_guide_cfgs([GC.load_guide_dict(1)], B, T)
            guide = IntersectionVolumeGuide(scene, ctx, cfgs, B)
            guide._bind()
            us = []
            for rep in range(WARMUP + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ctx.sync()
                e0.record(ctx.stream)
                for _ in range(calls):
                    _capi.check(ctx.lib.edmp_guide_gradient_dev(ctx.h, ptr(q), B, N - 2, _capi.as_pd(start), _capi.as_pd(goal), 100, ptr(grad), None))
                e1.record(ctx.stream)
                ctx.sync()
                if rep >= WARMUP:
                    us.append(1e3 * e0.elapsed_time(e1) / calls)
            per[k] = us
        base = float(np.median(per[0]))
        out[f"obstacles_{n_obstacles}"] = {f"sdf_rows_{k}": {"gradient_call_us": {"median": float(np.median(per[k])), "min": float(min(per[k])), "max": float(max(per[k]))},
                                                              "sdf_guide_kernel_us_median": float(np.median(per[k])) - base} for k in (171, 1024)}
        out[f"obstacles_{n_obstacles}"]["gradient_call_without_sdf_rows_us"] = {"median": base, "min": float(min(per[0])), "max": float(max(per[0]))}
    out["note"] = ("gradient_call_us: one edmp_guide_gradient_dev (start / goal upload, guide_kernel over all rows, sdf_guide_kernel over the SDF rows, norm, mix) in a "
                   f"chain of {calls} calls between two events; sdf_guide_kernel_us_median = that median minus the median of the same call without SDF rows")
    return out


def group_times(dif, ctx, reps, k=4, n_obstacles=16):
    """k scenes with SDF rows: one launch chain per scene against one chain for the group (both leave the state on the device)"""
    import numpy as np
    import torch

    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch
    from edmp_amd.temporalunet import TemporalUNet

    guides_of = FLAGSHIP[:-1] + (101,)
    cfgs = GC.build_guide_cfgs([GC.load_guide_dict(g) for g in guides_of], 0, T, rows_per_guide=GC.split_rows(B, len(guides_of)))
    net = TemporalUNet(None, C, 32, ctx, dims=(32, 64, 128, 256, 512, 512), seed=1, max_batch=k * B)
    guides = [IntersectionVolumeGuide(scenes.random_scene(11 + s, n_obstacles), ctx, cfgs, B) for s in range(k)]
    batch = SceneBatch(guides)
    rs = np.random.RandomState(99)
    noises = [ctx.to_dev(rs.standard_normal((T + 1, B, C, N)), torch.float64) for _ in range(k)]
    starts, goals = np.tile(scenes.DEFAULT_START, (k, 1)), np.tile(scenes.DEFAULT_GOAL, (k, 1))

    def serial():
        for s, g in enumerate(guides):
            dif.denoise_guided(net, g, N, C, cfgs["guidance_schedule"], batch_size=B, start=starts[s], goal=goals[s], noise=noises[s], return_device=True)

    def group():
        dif.denoise_guided_scenes(net, batch, N, C, starts, goals, noise=noises, return_device=True)

    out = {"scenes": k, "rows_per_scene": B, "obstacles": n_obstacles, "guides": list(guides_of), "sdf_rows_per_scene": int(cfgs["sdf_rows"].sum())}
    for name, fn in (("k1", serial), (f"k{k}", group)):
        ms = []
        for r in range(WARMUP + reps):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            if r >= WARMUP:
                ms.append(1e3 * (time.perf_counter() - t0))
        out[name] = spread(ms)
    out[f"k1_over_k{k}"] = out["k1"]["median_ms"] / out[f"k{k}"]["median_ms"]
    out["note"] = f"time of all {k} scenes: k1 = {k} denoise_guided calls in turn, k{k} = one denoise_guided_scenes call on the SceneBatch (the k noise streams are placed in the batch layout inside the call)"
    return out


def child(root, reps):
    """the flagship plan alone, with the package of `root`: prints one JSON line"""
    sys.path.insert(0, root)
    net, dif, ctx, noise = setup()
    print(json.dumps(plan_times(net, dif, ctx, noise, FLAGSHIP, 16, reps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-root", type=str, default=None, help="a built checkout of the parent commit: time the flagship plan there too")
    ap.add_argument("--only", choices=("group",), default=None, help="run one leg alone")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child-root", type=str, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("at least 20 timed calls per figure")
    if a.child_root:
        return child(a.child_root, a.reps)
    out = {"batch": B, "steps": T, "guided_steps": sum(1 for t in range(1, T + 1) if t % 2 == 0 and t >= 5), "warmup": WARMUP, "reps": a.reps,
           "clock": "plans: host wall time around a synchronised denoise_guided call (noise resident, state stays on the device); kernel: HIP events on the context's stream"}
    if a.parent_root:
        runs = []
        for name in ("parent", "this", "parent", "this"):
            root = a.parent_root if name == "parent" else HERE
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-root", root, "--reps", str(a.reps)], check=True, capture_output=True, text=True, timeout=600)
            runs.append({"tree": name, **json.loads(r.stdout.strip().splitlines()[-1])})
        out["flagship_parent_vs_this"] = runs
        med = {n: [r["median_ms"] for r in runs if r["tree"] == n] for n in ("parent", "this")}
        noise_ms = max(abs(med["parent"][0] - med["parent"][1]), abs(med["this"][0] - med["this"][1]), max(r["max_ms"] - r["min_ms"] for r in runs))
        out["flagship_agree_within_spread"] = bool(abs(sum(med["this"]) / 2 - sum(med["parent"]) / 2) <= noise_ms)
        out["flagship_spread_ms"] = noise_ms
    sys.path.insert(0, HERE)
    if a.only == "group":
        from edmp_amd.diffusion import Diffusion

        dif = Diffusion(T, "cuda:0")
        out["group"] = group_times(dif, dif.ctx, a.reps)
        txt = json.dumps(out)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
    net, dif, ctx, noise = setup()
    swapped = FLAGSHIP[:-1] + (101,)
    for n_obstacles in (16, 64):
        six = plan_times(net, dif, ctx, noise, FLAGSHIP, n_obstacles, a.reps)
        sdf = plan_times(net, dif, ctx, noise, swapped, n_obstacles, a.reps)
        out[f"plan_obstacles_{n_obstacles}"] = {"six_guides": six, "guide_10_replaced_by_101": sdf,
                                                "extra_us_per_guided_step": 1e3 * (sdf["median_ms"] - six["median_ms"]) / out["guided_steps"]}
    out["kernel"] = kernel_times(ctx, a.reps)
    del net, noise
    out["group"] = group_times(dif, ctx, a.reps)
    out["guide_kernel_us_per_launch_design_md"] = 28
    txt = json.dumps(out)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
