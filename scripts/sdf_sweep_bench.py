#!/usr/bin/env python
"""sdf_sweep_bench.py — what the SDF guide's swept-clearance term (sdf_sweep_kernel, csrc/sdf.hip) costs: the guide's part of one guided
step (edmp_guide_gradient_dev on a device tensor of 1024 x (7, 48) interior waypoints, t = 100) of the ensemble (1, 104), half the rows
each, with sweep_substeps K = 2, 4 and 8, against the same ensemble with guide 104's sweep weight set to 0 (no sweep keys, nothing more
launched than before the term existed).

    python scripts/sdf_sweep_bench.py [--rows 1024] [--calls 20] [--inner 20] [--warmup 3] [--out profiles/sdf_sweep_bench.json]

The guides live in their own resident slots and are measured alternately in one process, so all see the same box and the same clocks.
A sample is `inner` back-to-back calls, timed by a host clock that ends in a device synchronise (one call is a fraction of a
millisecond: a single one would measure the clock); each figure is the median of `calls` samples after `warmup`, per call.  The binding
of a guide's slot happens outside the timed window.

Prints ONE JSON line and writes it to --out.  Informative: no time is gated, and this is never bench.py's value."""
from __future__ import annotations

import argparse
import copy
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
SUBSTEPS = (2, 4, 8)


def measure(rows=1024, calls=20, inner=20, warmup=3, device="cuda:0", commit=None):
    import torch

    from edmp_amd import _capi, scenes
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import ptr

    base = GC.load_guide_dict(104)
    dicts = {"sweep_weight_0": copy.deepcopy(base)}
    dicts["sweep_weight_0"]["hyperparameters"]["sdf"]["sweep_weight"] = 0.0
    for K in SUBSTEPS:
        dicts[f"K{K}"] = copy.deepcopy(base)
        dicts[f"K{K}"]["hyperparameters"]["sdf"]["sweep_substeps"] = K
    s, g = np.ascontiguousarray(scenes.DEFAULT_START, dtype=np.float64), np.ascontiguousarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    guides = {}
    for name, d in dicts.items():
        cfgs = GC.build_guide_cfgs([GC.load_guide_dict(1), d], rows // 2, T)
        guides[name] = IntersectionVolumeGuide(scenes.random_scene(11, 16), device, cfgs, cfgs["total_batch_size"])
    assert not guides["sweep_weight_0"].has_sweep_term and all(guides[f"K{K}"].has_sweep_term for K in SUBSTEPS)
    B = guides["K4"].batch_size
    ctx = guides["K4"].ctx
    t = np.linspace(0, 1, N)[1:-1]
    X = s[None, :, None] * (1 - t) + g[None, :, None] * t + 0.1 * np.random.RandomState(3).standard_normal((B, 7, N - 2))
    ji = ctx.to_dev(np.ascontiguousarray(X), torch.float64)
    outs = {name: ctx.empty((B, 7, N - 2), torch.float64) for name in guides}

    def sample(name):
        guides[name]._bind()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(inner):
            _capi.check(ctx.lib.edmp_guide_gradient_dev(ctx.h, ptr(ji), B, N - 2, _capi.as_pd(s), _capi.as_pd(g), 100, ptr(outs[name]), None), "edmp_guide_gradient_dev")
        ctx.sync()
        return (time.perf_counter() - t0) / inner

    times = {name: [] for name in guides}
    for k in range(warmup + calls):
        for name in guides:  # alternating: all see the same box at the same time
            v = sample(name)
            if k >= warmup:
                times[name].append(v)
    G = {name: ctx.to_host(o) for name, o in outs.items()}
    half = B // 2
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        pass
    med = {name: statistics.median(v) for name, v in times.items()}
    return {
        "rows": B, "sweep_rows": half, "L": N - 2, "t": 100, "obstacles": 16, "calls": calls, "inner": inner, "warmup": warmup,
        "clock": "median of `calls` samples per guide, taken alternately; a sample is `inner` back-to-back edmp_guide_gradient_dev calls inside a host "
                 "perf_counter window that ends in a device synchronise, divided by `inner`",
        "guided_step_s": med,
        "guided_step_is": "edmp_guide_gradient_dev, ensemble (1, 104), half the rows each, (7, 48) interior waypoints on the device, t = 100; "
                          "sweep_weight_0: the same ensemble with guide 104's sweep_weight 0; K<n>: sweep_substeps n",
        "sweep_term_s": {f"K{K}": med[f"K{K}"] - med["sweep_weight_0"] for K in SUBSTEPS},
        "sweep_term_per_interpolant_s": {f"K{K}": (med[f"K{K}"] - med["sweep_weight_0"]) / (K - 1) for K in SUBSTEPS},
        "over_without": {f"K{K}": med[f"K{K}"] / med["sweep_weight_0"] for K in SUBSTEPS},
        "spread_s": {name: [min(v), max(v)] for name, v in times.items()},
        "unweighted_rows_bit_identical": bool(all(np.array_equal(G["sweep_weight_0"][:half], G[f"K{K}"][:half]) for K in SUBSTEPS)),
        "weighted_rows_differ": bool(all(not np.array_equal(G["sweep_weight_0"][half:], G[f"K{K}"][half:]) for K in SUBSTEPS)),
        "box": {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "torch": torch.__version__, "hip": torch.version.hip},
        "commit": commit, "commit_is": "the commit the measured working tree is based on",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sdf_sweep_bench.json"))
    ap.add_argument("--commit", type=str, default=None, help="commit the working tree is based on (default: git rev-parse, where the tree is a checkout)")
    a = ap.parse_args()
    out = measure(a.rows, calls=a.calls, inner=a.inner, warmup=a.warmup, commit=a.commit)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
