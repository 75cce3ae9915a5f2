#!/usr/bin/env python
"""repair_bench.py — what the repair stage (sdf_repair_kernel, csrc/sdf.hip) costs: edmp_sdf_repair_rows_dev on a device state of
1024 x (7, 50) rows among 16 obstacles at substeps K = 4 with iters = 1, 8 and 32, at a margin so large (1 m) that no row stops early -
every row runs iters updates and iters + 1 evaluations in ONE launch.

    python scripts/repair_bench.py [--rows 1024] [--calls 20] [--warmup 3] [--out profiles/repair_bench.json]

A sample is one call on a fresh device copy of the state (the copy is made and synchronised outside the timed window; the entry point
itself ends in a stream synchronise), timed by a host clock; each figure is the median of `calls` samples after `warmup`, the three
iteration counts taken alternately.  The time per iteration is the slope between iters = 1 and iters = 32.  For comparison README's
measured 164.2 us: sdf_guide_kernel + sdf_sweep_kernel (one evaluation with its gradient, no update) at K = 4 on 512 rows.

Prints ONE JSON line and writes it to --out.  Informative: no time is gated, and this is never bench.py's value."""
from __future__ import annotations

import argparse
import ctypes as C
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
ITERS = (1, 8, 32)
MARGIN = 1.0
GUIDED_STEP_K4_512_ROWS_S = 164.2e-6  # README: the guide's part of a guided step, ensemble 1 + 104, K = 4 (profiles/sdf_sweep_bench.json)


def measure(rows=1024, calls=20, warmup=3, device="cuda:0", commit=None):
    import torch

    from edmp_amd import _capi, scenes
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import ptr

    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(1)], rows, T)
    guide = IntersectionVolumeGuide(scenes.random_scene(11, 16), device, cfgs, rows)
    guide._bind_sdf()
    ctx = guide.ctx
    s, g = np.ascontiguousarray(scenes.DEFAULT_START, dtype=np.float64), np.ascontiguousarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    t = np.linspace(0, 1, N)
    X = s[None, :, None] * (1 - t) + g[None, :, None] * t + 0.1 * np.random.RandomState(3).standard_normal((rows, 7, N))
    X[:, :, 0], X[:, :, -1] = s, g
    X0 = ctx.to_dev(np.ascontiguousarray(X), torch.float64)
    rep, its = ctx.empty((2, rows, 2), torch.float64), ctx.empty((rows,), torch.int32)

    def sample(iters):
        with torch.cuda.stream(ctx.stream):
            Xw = X0.clone()
        ctx.sync()
        t0 = time.perf_counter()
        _capi.check(ctx.lib.edmp_sdf_repair_rows_dev(ctx.h, ptr(Xw), rows, N, _capi.as_pd(s), _capi.as_pd(g), None, 0, K, iters, MARGIN, 0.5, 0.02, 0.02,
                                                     C.c_void_p(rep[0].data_ptr()), C.c_void_p(rep[1].data_ptr()), ptr(its)), "edmp_sdf_repair_rows_dev")
        dt = time.perf_counter() - t0
        return dt, ctx.to_host(its)

    times = {n: [] for n in ITERS}
    full = True
    for k in range(warmup + calls):
        for n in ITERS:  # alternating: all see the same box at the same time
            dt, done = sample(n)
            full = full and bool((done == n).all())
            if k >= warmup:
                times[n].append(dt)
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        pass
    med = {n: statistics.median(v) for n, v in times.items()}
    per_iter = (med[ITERS[-1]] - med[ITERS[0]]) / (ITERS[-1] - ITERS[0])
    return {
        "rows": rows, "N": N, "L": N - 2, "obstacles": 16, "substeps": K, "margin": MARGIN, "smoothness": 0.5, "step": 0.02, "max_step": 0.02, "calls": calls,
        "warmup": warmup,
        "clock": "median of `calls` samples per iteration count, taken alternately; a sample is ONE edmp_sdf_repair_rows_dev call (it ends in a stream "
                 "synchronise) on a fresh device copy of the state inside a host perf_counter window",
        "call_s": {f"iters{n}": med[n] for n in ITERS},
        "per_iteration_s": per_iter,
        "per_iteration_is": "the slope between iters = 1 and iters = 32: one evaluation with its gradient plus one update of every row, no launch",
        "call_over_evaluations_s": {f"iters{n}": med[n] / (n + 1) for n in ITERS},
        "spread_s": {f"iters{n}": [min(v), max(v)] for n, v in times.items()},
        "every_row_ran_all_iterations": full,
        "for_comparison_guided_step_K4_512_rows_s": GUIDED_STEP_K4_512_ROWS_S,
        "for_comparison_is": "README: sdf_guide_kernel + sdf_sweep_kernel inside edmp_guide_gradient_dev, ensemble 1 + 104, 512 SDF rows, K = 4 - one evaluation "
                             "with its gradient on half as many rows, measured on another day",
        "box": {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "torch": torch.__version__, "hip": torch.version.hip},
        "commit": commit, "commit_is": "the commit the measured working tree is based on",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "repair_bench.json"))
    ap.add_argument("--commit", type=str, default=None, help="commit the working tree is based on (default: git rev-parse, where the tree is a checkout)")
    a = ap.parse_args()
    out = measure(a.rows, calls=a.calls, warmup=a.warmup, commit=a.commit)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
