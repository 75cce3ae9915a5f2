#!/usr/bin/env python
"""self_collision_bench.py — what the self-collision check of a whole batch costs: IntersectionVolumeGuide.self_collision_rows
(edmp_self_collision_rows_dev, csrc/selfcol.hip) on 1024 x (7, 50) rows from a device tensor, against the NumPy reference loop on the
same box (oracle.success_oracle's link-box poses and separating-axis test over the same configurations and pairs) and against
success_rows on the same rows.

    python scripts/self_collision_bench.py [--rows 1024] [--calls 20] [--warmup 3] [--out profiles/self_collision_bench.json]

Rows: straight joint-space lines between two configurations uniform in the joint limits plus 0.02 * randn (the recipe of
tests/self_collision_inputs.py, RandomState(7)): about a quarter of them collide, so the kernel's early exit and its full walk are both
in the mix; `rows_free_only_s` times the free rows alone - the worst case, every (configuration, pair) tested.  Each figure is the median
of `calls` calls, each call timed by a host clock that ends in a device synchronise, after `warmup` calls.

Second measurement, what the SDF guide's self-clearance term costs: the guide's part of one guided step (edmp_guide_gradient_dev on a
device tensor of `rows` x (7, 48) interior waypoints, t = 100) of the ensemble (1, 101) against the same with sample guide 102 in place
of 101.  `--step-only 101` measures that one figure alone and uses nothing newer than get_gradient's entry point, so the same file run on
the parent commit gives the figure to pass here as --parent-step-101-s: the unweighted path should cost what it cost there.

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

T, N = 255, 50


def numpy_reference(X, substeps, mask):
    """first / pair / free as tests/self_collision_inputs.reference computes them, without its decision-distance pass"""
    from edmp_amd import franka
    from oracle import success_oracle as SO

    n, S = X.shape[0], int(substeps)
    nc = (X.shape[2] - 1) * S + 1
    Q = np.zeros((n, nc, 7))
    for i in range(X.shape[2]):
        for s in range(S if i < X.shape[2] - 1 else 1):
            f = s / S
            Q[:, i * S + s] = X[:, :, i] if s == 0 else (1 - f) * X[:, :, i] + f * X[:, :, i + 1]
    he = franka.link_half_extents().astype(np.float64)
    Rl, cl = SO.link_box_poses_batch(Q.reshape(-1, 7))
    big = np.iinfo(np.int64).max
    key = np.full(n * nc, big, dtype=np.int64)
    cidx = np.tile(np.arange(nc, dtype=np.int64), n)
    for a in range(9):
        for b in range(a + 1, 9):
            if mask[a][b]:
                hit = SO.obb_overlap_batch(Rl[:, a], cl[:, a], he[a], Rl[:, b], cl[:, b], he[b])
                key = np.where(hit, np.minimum(key, cidx * 81 + a * 9 + b), key)
    key = key.reshape(n, nc).min(axis=1)
    free = key == big
    k = np.where(free, 0, key)
    return np.where(free, -1, (k // 81) // S).astype(np.int32), np.where(free, -1, k % 81).astype(np.int32), free


def guided_step_s(sdf_guide, rows=1024, calls=20, warmup=3, device="cuda:0"):
    """median seconds of the guide's part of one guided step, ensemble (1, sdf_guide), half the rows each"""
    import torch

    from edmp_amd import _capi, scenes
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import ptr

    cfgs = GC.build_guide_cfgs([GC.load_guide_dict(1), GC.load_guide_dict(int(sdf_guide))], rows // 2, T)
    B = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(scenes.random_scene(11, 16), device, cfgs, B)
    ctx = guide.ctx
    s, g = np.ascontiguousarray(scenes.DEFAULT_START, dtype=np.float64), np.ascontiguousarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    t = np.linspace(0, 1, N)[1:-1]
    X = s[None, :, None] * (1 - t) + g[None, :, None] * t + 0.1 * np.random.RandomState(3).standard_normal((B, 7, N - 2))
    ji, out = ctx.to_dev(np.ascontiguousarray(X), torch.float64), ctx.empty((B, 7, N - 2), torch.float64)
    guide._bind()
    times = []
    for k in range(warmup + calls):
        t0 = time.perf_counter()
        _capi.check(ctx.lib.edmp_guide_gradient_dev(ctx.h, ptr(ji), B, N - 2, _capi.as_pd(s), _capi.as_pd(g), 100, ptr(out), None), "edmp_guide_gradient_dev")
        ctx.sync()
        if k >= warmup:
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


def measure(rows=1024, calls=20, warmup=3, substeps=4, device="cuda:0", commit=None):
    import torch

    from edmp_amd import franka, scenes
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide

    rs = np.random.RandomState(7)
    lo, hi = franka.joint_limits()
    a, b = rs.uniform(lo, hi, (rows, 7)), rs.uniform(lo, hi, (rows, 7))
    t = np.linspace(0, 1, N)
    X = np.ascontiguousarray(a[:, :, None] * (1 - t) + b[:, :, None] * t + 0.02 * rs.standard_normal((rows, 7, N)))
    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(1)], rows, T)
    guide = IntersectionVolumeGuide(scenes.random_scene(11, 16), device, cfgs, rows)
    Xd = torch.from_numpy(X).to(device)
    mask = franka.self_collision_pairs()

    def clock(fn, n_calls=calls, n_warm=warmup):
        for _ in range(n_warm):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(n_calls):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return statistics.median(out)

    res = guide.self_collision_rows(Xd, substeps=substeps)
    t0 = time.perf_counter()
    ref_first, ref_pair, ref_free = numpy_reference(X, substeps, mask)
    numpy_s = time.perf_counter() - t0
    same = bool(np.array_equal(res["first"], ref_first) and np.array_equal(res["pair"][:, 0] * 9 + res["pair"][:, 1], np.where(ref_free, -10, ref_pair))
                and np.array_equal(res["free"], ref_free))
    Xfree = Xd[torch.from_numpy(np.flatnonzero(ref_free)).to(device)].contiguous()
    check_s = clock(lambda: guide.self_collision_rows(Xd, substeps=substeps, return_device=True))
    free_s = clock(lambda: guide.self_collision_rows(Xfree, substeps=substeps, return_device=True))
    host_s = clock(lambda: guide.self_collision_rows(X, substeps=substeps))
    success_s = clock(lambda: guide.success_rows(Xd, substeps=substeps, return_device=True))
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        pass
    return {
        "rows": rows, "N": N, "substeps": substeps, "pairs": int(mask.sum()), "rows_free": int(ref_free.sum()), "calls": calls, "warmup": warmup,
        "clock": "median of `calls` calls, each a host perf_counter around one call ending in torch.cuda.synchronize(), after `warmup` calls",
        "self_collision_rows_device_input_s": check_s, "self_collision_rows_free_only_s": free_s, "rows_free_only": int(Xfree.shape[0]),
        "self_collision_rows_host_input_s": host_s,
        "success_rows_device_input_s": success_s, "success_rows_is": "the same rows against a 16-cuboid synthetic scene, return_device=True (its counts are read back)",
        "numpy_reference_s": numpy_s, "numpy_reference_is": "oracle link_box_poses_batch + obb_overlap_batch over the same configurations and pairs, once, this box's CPU",
        "numpy_over_device_input": numpy_s / check_s, "equal_to_numpy_reference": same,
        "guided_step_guide_101_s": guided_step_s(101, rows, calls, warmup, device), "guided_step_guide_102_s": guided_step_s(102, rows, calls, warmup, device),
        "guided_step_is": "edmp_guide_gradient_dev, ensemble (1, 101 or 102), half the rows each, (7, 48) interior waypoints on the device, t = 100",
        "box": {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "torch": torch.__version__, "hip": torch.version.hip},
        "commit": commit, "commit_is": "the commit the measured working tree is based on",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "self_collision_bench.json"))
    ap.add_argument("--commit", type=str, default=None, help="commit the working tree is based on (default: git rev-parse, where the tree is a checkout)")
    ap.add_argument("--step-only", type=int, default=None, help="measure the guided step of the ensemble (1, this guide) alone and print it")
    ap.add_argument("--parent-step-101-s", type=float, default=None, help="--step-only 101 as measured on the parent commit, recorded beside this commit's")
    a = ap.parse_args()
    if a.step_only is not None:
        print(json.dumps({f"guided_step_guide_{a.step_only}_s": guided_step_s(a.step_only, a.rows, a.calls, a.warmup)}))
        return
    out = measure(a.rows, calls=a.calls, warmup=a.warmup, commit=a.commit)
    out["guided_step_guide_101_parent_commit_s"] = a.parent_step_101_s  # None: not measured
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
