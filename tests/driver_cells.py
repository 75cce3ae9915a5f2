"""The cells of tests/golden/driver_parent.json, defined once: what one infer_serial.run call returns, prints and asks of the library, for a
fixed set of option combinations on configs/cfg_c1_plumbing.yaml (4 rows per guide, T = 255) and two or three seeded "stress" scenes.
scripts/record_driver_parent.py evaluates them with the PARENT commit's infer_serial.py and package, tests/test_gpu_driver_record.py
with this checkout's, and holds the two equal: a restructuring of the driver changes no key, no key order, no type, no value, no printed
line, no draw from the global RandomState and, per context, no library call or its place in the sequence.  infer_serial and edmp_amd
are whatever sys.path finds first."""
import contextlib
import hashlib
import io
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "driver_parent.json")
DEV = "cuda:0"
TIMES = ("timings", "planning_time_s", "scene_wall_s", "done_at")  # wall-clock values: their keys and types are recorded, not their values
ALL = dict(ensemble_report=True, prefer="shortest", self_collision=True, repair=6, repair_margin=0.03)
#        name: (guides of the config, scenes, problem set from target poses, run()'s options)
CELLS = {"plain_serial": ([1], 2, False, {}),
         "plain_group": ([1], 3, False, dict(scenes_per_launch=2)),  # (a leftover group of one)
         "plain_in_flight": ([1], 3, False, dict(scenes_in_flight=2)),
         "all_serial": ([1, 102, 103, 104], 2, False, ALL),
         "all_group": ([1, 102, 103, 104], 3, False, dict(ALL, scenes_per_launch=2)),
         "report_serial": ([1, 104], 2, False, dict(ensemble_report=True)),  # (no `prefer`: the metrics are the scoring step's own call)
         "report_group": ([1, 104], 2, False, dict(ensemble_report=True, scenes_per_launch=2)),
         "device_noise_serial": ([1], 2, False, dict(device_noise=11)),
         "device_noise_group": ([1], 3, False, dict(device_noise=11, scenes_per_launch=2)),
         "ik_serial": ([1], 2, True, dict(ik_seeds=128)),
         "ik_group": ([1], 2, True, dict(ik_seeds=128, scenes_per_launch=2))}
OPTIONAL_KEYS = ("scenes_in_launch", "noise_seed", "min_clearance", "min_swept_clearance", "min_self_clearance", "position_error", "orientation_error", "self_collision_free",
                 "rows_self_collision_free", "first_self_collision_waypoint", "self_collision_pair", "rows_repaired", "rows_repair_clear", "repair_iters", "prefer", "ensemble")
OPTIONAL_TIMINGS = ("noise_wait_s", "repair_s", "batch_metrics_s", "denoise_s_is", "guide_ctor_s_is", "ik_filter_s_is")


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


def frozen(v):
    """a result value as JSON that loses nothing: floats as TYPE:hex, arrays as the SHA-256 of dtype, shape and bytes, dicts as ordered pairs"""
    if isinstance(v, np.ndarray):
        return {"array": sha(v)}
    if isinstance(v, (float, np.floating)):
        return f"{type(v).__name__}:{float(v).hex()}"
    if isinstance(v, (np.integer, np.bool_)):
        return f"{type(v).__name__}:{int(v)}"
    if isinstance(v, dict):
        return [[k, frozen(x)] for k, x in v.items()]
    if isinstance(v, (list, tuple)):
        return [type(v).__name__] + [frozen(x) for x in v]
    assert v is None or isinstance(v, (bool, int, str)), type(v)
    return v


def problem_set(tmp):
    """the target-pose problem set of tests/test_gpu_ik.py: two problems that carry a target and no IK goals -> ProblemSetDataset"""
    from edmp_amd import franka, scenes
    from tests import ik_inputs as I

    lo, hi = franka.joint_limits()
    rs = np.random.RandomState(9)
    wxyz = lambda o: [float(o[6]), float(o[3]), float(o[4]), float(o[5])]  # noqa: E731
    problems = []
    for k in range(2):
        oc, tg = scenes.random_scene(20 + k, 6), I.targets()[k]
        problems.append({"cuboids": [{"center": o[:3].tolist(), "quaternion_wxyz": wxyz(o), "dims": o[7:10].tolist()} for o in oc[:4]],
                         "cylinders": [{"center": o[:3].tolist(), "quaternion_wxyz": wxyz(o), "radius": float(o[7]), "height": float(o[9])} for o in oc[4:]],
                         "start": rs.uniform(lo, hi).tolist(), "target": {"xyz": tg[:3, 3].tolist(), "quaternion_wxyz": I.quaternion_wxyz(tg[:3, :3]), "frame": "end_effector"}})
    path = os.path.join(tmp, "problems.json")
    with open(path, "w") as f:
        json.dump({"format": "edmp_amd problem set v1", "scene_types": {"tabletop": problems}}, f)
    return scenes.ProblemSetDataset(path)


class Spy:
    """stands in for a context's `lib`: forwards everything, notes the name of every edmp_* entry point as it is called"""

    def __init__(self, lib):
        self.__dict__.update(lib=lib, calls=[])

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("edmp_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def run_lengths(names):
    """the sequence as [name, repeats] runs"""
    out = []
    for n in names:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return out


def evaluate(name, tmp):
    """run the cell `name` (its config is written under the directory tmp) -> its record"""
    import yaml

    import infer_serial
    from edmp_amd import scenes
    from edmp_amd.runtime import get_context, lane_context

    guides, n_scenes, from_targets, kw = CELLS[name]
    tmp = str(tmp)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cfg_c1_plumbing.yaml")))
    cfg["guide"]["guides"] = list(guides)
    if from_targets:
        cfg["dataset"]["scene_types"] = ["tabletop"]
    os.makedirs(os.path.join(tmp, "cfgs"), exist_ok=True)
    path = os.path.join(tmp, "cfgs", f"{name}.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    np.random.seed(31)
    ds = problem_set(tmp) if from_targets else scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=n_scenes, n_obstacles=6, n_cylinders=1)
    base = get_context(DEV)
    ctxs = {"base": base, "lane1": lane_context(base, 1)}
    spies = {k: Spy(c.lib) for k, c in ctxs.items()}
    infer_serial.run.last_summary = None
    out = io.StringIO()
    try:
        for k, c in ctxs.items():
            c.lib = spies[k]
            c.sampler_T = c.bound_model = c.bound_guide = None  # (what is resident is asked for again: the calls do not depend on what the context ran before)
        with contextlib.redirect_stdout(out):
            results = infer_serial.run(path, dataset=ds, verbose=True, **kw)
    finally:
        for k, c in ctxs.items():
            c.lib = spies[k].lib
    state = np.random.get_state()
    summary = dict(infer_serial.run.last_summary)
    summary.pop("planning_time_s")
    return {"scenes": [{"keys": list(r), "types": {k: type(v).__name__ for k, v in r.items()}, "values": {k: frozen(v) for k, v in r.items() if k not in TIMES},
                        "timings": [[k, v if isinstance(v, str) else type(v).__name__] for k, v in r["timings"].items()]} for r in results],
            "printed": [re.sub(r"\d+\.\d+ s", "# s", line) for line in out.getvalue().splitlines()],
            "summary": frozen(summary),
            "random_state": [state[0], sha(state[1]), int(state[2]), int(state[3]), float(state[4]).hex()],
            "calls": {k: run_lengths(s.calls) for k, s in spies.items()}}
