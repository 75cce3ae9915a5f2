#!/usr/bin/env python
"""blend_bench.py — what the corner blends (csrc/blend.hip) buy and cost.

    python scripts/blend_bench.py [--rows 1024] [--calls 20] [--warmup 3] [--out profiles/blend_bench.json]

B = 1024, N = 50, 16 obstacles, the bumped zigzag rows of scripts/shortcut_bench.py as they stand and after shortcut_rows (passes = 4,
K = 4).  Per state: edmp_blend_rows_dev (deviation 10 mrad, reach 0.4, substeps 4, halvings 2 - the illustrative defaults),
edmp_time_blended_rows_dev on its beta and edmp_sample_blended_rows_dev at a 1 ms period for the first 64 rows; the census of the corner
codes; the durations of the unblended (edmp_time_rows_dev) and of the blended motion, mean and median.

A sample is ONE call followed by the context's synchronise (the blend and sample calls end in one themselves) inside a host perf_counter
window; each figure is the median of `calls` samples after `warmup`.  Prints ONE JSON line and writes it to --out.  Informative: no time
is gated, and this is never bench.py's value.

With --self-safe-out FILE the script runs ONE other leg instead: guide.blend_rows on the same two states with self_pairs=None and
self_pairs=True (the self-collision test of the tries, blend_rows_kernel<true>), the two taken alternately, medians of `calls` calls each
with the context's synchronise, with the rejected counts; the record goes under "blend" into FILE (profiles/self_safe_bench.json, which
scripts/shortcut_bench.py shares)."""
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

T, N, K, PASSES, PERIOD = 255, 50, 4, 4, 1e-3
DEVIATION, REACH, SUBSTEPS, HALVINGS = 0.01, 0.4, 4, 2
SCENE_SEED, SCENE_SCALE = 12, 0.35  # (scripts/shortcut_bench.py's scene)


def measure(rows=1024, calls=20, warmup=3, device="cuda:0", commit=None):
    import torch

    from edmp_amd import _capi, franka, scenes
    from edmp_amd import evaluation as EV
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import ptr

    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(1)], rows, T)
    scene = scenes.random_scene(SCENE_SEED, 16)
    scene[:, 7:10] *= SCENE_SCALE
    guide = IntersectionVolumeGuide(scene, device, cfgs, rows)
    ctx = guide.ctx
    s, g = np.ascontiguousarray(scenes.DEFAULT_START, dtype=np.float64), np.ascontiguousarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    f = np.linspace(0, 1, N)
    rs = np.random.RandomState(3)
    X = s[None, :, None] * (1 - f) + g[None, :, None] * f + rs.uniform(-0.6, 0.6, size=(rows, 7, 1)) * np.sin(np.pi * f)[None, None, :]
    X[:, 3, 1:-1] += 0.1 * (-1.0) ** np.arange(1, N - 1)
    X[:, :, 0], X[:, :, -1] = s, g
    states = {"sampler_like": ctx.to_dev(np.ascontiguousarray(X), torch.float64)}
    states["after_shortcut"] = guide.shortcut_rows(states["sampler_like"], passes=PASSES, substeps=K, log_cap=0, return_device=True)["trajectories"].contiguous()
    lim = [np.ascontiguousarray(v) for v in franka.timing_limits()]
    dev, dh = np.full(7, DEVIATION), np.ascontiguousarray(franka.dh_table_f64())
    beta, code, halved, tested = ctx.empty((rows, N), torch.float64), ctx.empty((rows, N), torch.int32), ctx.empty((rows, N), torch.int32), ctx.empty((rows,), torch.int32)
    prof = {k: ctx.empty(shape, torch.int32 if k == "limit" else torch.float64)
            for k, shape in (("y", (rows, N)), ("phase", (rows, N - 1, 3)), ("times", (rows, N, 2)), ("duration", (rows,)), ("limit", (rows, N)), ("seg", (rows, N - 1, 2)),
                             ("blend", (rows, N)))}
    guide._bind()
    lib = ctx.lib

    def timed(fn):
        dts = []
        for _ in range(warmup + calls):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            dts.append(time.perf_counter() - t0)
        dts = dts[warmup:]
        return dict(call_s=statistics.median(dts), spread_s=[min(dts), max(dts)])

    def stats(d):
        return dict(mean=float(d.mean()), median=float(np.median(d)), min=float(d.min()), max=float(d.max()))

    out = {}
    for name, Xd in states.items():
        plain = ctx.to_host(EV.time_rows_on(ctx, Xd, return_device=True)["duration"])
        rec = {"blend_rows": timed(lambda: _capi.check(lib.edmp_blend_rows_dev(
            ctx.h, ptr(Xd), rows, N, None, 0, *(_capi.as_pd(v) for v in lim), _capi.as_pd(dev), REACH, SUBSTEPS, HALVINGS, _capi.as_pd(dh), ptr(beta), ptr(code), ptr(halved),
            ptr(tested)), "edmp_blend_rows_dev"))}
        rec["time_blended_rows"] = timed(lambda: _capi.check(lib.edmp_time_blended_rows_dev(
            ctx.h, ptr(Xd), rows, N, ptr(beta), *(_capi.as_pd(v) for v in lim), *(ptr(prof[k]) for k in EV.BLENDED_PROFILE_KEYS)), "edmp_time_blended_rows_dev"))
        blended = ctx.to_host(prof["duration"])
        R = min(64, rows)
        M = max(EV.sample_count(v, PERIOD) for v in blended[:R])
        q, qd, cnt = ctx.empty((R, 7, M), torch.float64), ctx.empty((R, 7, M), torch.float64), ctx.empty((R,), torch.int32)
        listed = np.arange(R, dtype=np.int32)
        rec["sample_blended_rows"] = dict(timed(lambda: _capi.check(lib.edmp_sample_blended_rows_dev(
            ctx.h, ptr(Xd), rows, N, ptr(beta), ptr(prof["y"]), ptr(prof["phase"]), ptr(prof["times"]), ptr(prof["duration"]), ptr(prof["seg"]), _capi.as_pi32(listed), R,
            PERIOD, M, ptr(q), ptr(qd), ptr(cnt)), "edmp_sample_blended_rows_dev")), rows=R, M=M, period_s=PERIOD, bytes_written=2 * R * 7 * M * 8 + 4 * R)
        del q, qd
        c = ctx.to_host(code)[:, 1:-1]
        rec.update(corner_codes={nm: int((c == k).sum()) for k, nm in enumerate(EV.BLEND_CODE_NAMES)}, rows_left_alone=int((ctx.to_host(code)[:, 0] == -1).sum()),
                   configurations_tested=int(ctx.to_host(tested).sum()), halved={str(h): int(((ctx.to_host(halved)[:, 1:-1] == h) & (c == 3)).sum()) for h in range(HALVINGS + 1)},
                   duration_s=stats(plain), blended_duration_s=stats(blended), rows_faster=int((blended < plain).sum()), rows_slower=int((blended > plain).sum()))
        out[name] = rec
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        pass
    return {
        "rows": rows, "N": N, "limits": "franka.timing_limits(): published joint velocity / acceleration limits, corner jump = amax x 1 ms (illustrative)",
        "blend": f"deviation {DEVIATION} rad, reach {REACH}, substeps {SUBSTEPS}, halvings {HALVINGS} (illustrative defaults)",
        "shortcut": f"shortcut_rows(passes={PASSES}, substeps={K}) among 16 obstacles (scenes.random_scene({SCENE_SEED}, 16), extents x {SCENE_SCALE})", "calls": calls, "warmup": warmup,
        "clock": "median of `calls` samples; a sample is ONE entry-point call and the context's synchronise inside a host perf_counter window",
        "states": out,
        "box": {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "torch": torch.__version__, "hip": torch.version.hip},
        "commit": commit, "commit_is": "the commit the measured working tree is based on",
    }


def measure_self_safe(rows=1024, calls=20, warmup=3):
    """the self-safe leg: the same two states and scene (scripts/shortcut_bench.py: bench_state), guide.blend_rows with self_pairs=None and True"""
    import torch

    from shortcut_bench import alternate, bench_state  # (scripts/ is this script's directory)

    guide, X0 = bench_state(rows)
    states = {"sampler_like": X0,
              "after_shortcut": guide.shortcut_rows(X0, passes=PASSES, substeps=K, log_cap=0, return_device=True)["trajectories"].contiguous()}
    out = {}
    for name, Xd in states.items():
        med, spread, last = alternate(guide.ctx, lambda pairs: guide.blend_rows(Xd, deviation=DEVIATION, reach=REACH, substeps=SUBSTEPS, halvings=HALVINGS, return_device=True,
                                                                                self_pairs=pairs), calls, warmup)
        out[name] = {"call_s": med, "spread_s": spread, "on_over_off": med["on"] / med["off"],
                     "configurations_tested": {k: int(v["tested"].sum()) for k, v in last.items()}, "blended": {k: int((v["code"] == 3).sum()) for k, v in last.items()},
                     "self_hits": int(last["on"]["self_hits"].sum()), "codes_equal": bool(torch.equal(last["on"]["code"], last["off"]["code"]))}
    return {
        "rows": rows, "N": N, "obstacles": 16, "blend": f"deviation {DEVIATION} rad, reach {REACH}, substeps {SUBSTEPS}, halvings {HALVINGS} (illustrative defaults)",
        "calls": calls, "warmup": warmup, "pair_mask": "franka.self_collision_pairs(): 18 pairs, 6 lower links",
        "clock": "median of `calls` guide.blend_rows(return_device=True) calls per leg, taken alternately, each with the context's synchronise inside a host perf_counter window",
        "states": out,
        "box": {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "torch": torch.__version__, "hip": torch.version.hip},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "blend_bench.json"))
    ap.add_argument("--commit", type=str, default=None, help="commit the working tree is based on (default: git rev-parse, where the tree is a checkout)")
    ap.add_argument("--self-safe-out", type=str, default=None, help="run the self-safe leg alone and put its record under \"blend\" into this JSON file")
    a = ap.parse_args()
    if a.self_safe_out:
        from shortcut_bench import merge_into  # (scripts/ is this script's directory)

        out = measure_self_safe(a.rows, calls=a.calls, warmup=a.warmup)
        print(json.dumps(out))
        merge_into(a.self_safe_out, "blend", out)
        return
    out = measure(a.rows, calls=a.calls, warmup=a.warmup, commit=a.commit)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
