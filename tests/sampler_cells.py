"""The cells of tests/golden/sampler_parent.json, defined once: what one Diffusion.denoise_guided / denoise_guided_scenes call returns, draws
from the global RandomState and asks of the library, for every noise form crossed with every run form, and every refusal of the two methods.
scripts/record_sampler_parent.py evaluates them with the PARENT commit's package, tests/test_gpu_sampler_record.py with this checkout's, and
holds the two equal: a restructuring of the two methods changes no result bit, no draw, no library call, none of its integer arguments, no
null pointer and no refusal's text.  edmp_amd is whatever sys.path finds first.

Shapes: T = 255, the tiny net (max_batch 18), 6 rows of guides [1, 10] x 3 per scene - a scene boundary falls inside a wave -, S = 3 scenes of
4, 7 and 10 obstacles, chunk_steps = 5 (12 steps: segments of 1, 2, 4 and 5).  Most cells run 12 steps - T .. T - 11 under t_stop, or 12 .. 1
from a warm start, which ends in the t == 1 step of quirk Q3 - and two per form the whole loop."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from tests.util import T, TINY_DIMS, cfgs_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "sampler_parent.json")
DEV = "cuda:0"
S, B, CN, STEPS, CHUNK = 3, 6, (7, 50), 12, 5
FORMS = ("single", "scenes")
NOISES = ("numpy", "host", "device", "pinned", "stream", "device_noise", "string")  # "string": noise="device" with seed=, the single form's alone
#      name: (denoise_guided* keywords, warm start: None or (renoise, x0 per row), what else the cell does)
RUNS = {"stop": (dict(t_stop=T - STEPS), None, None),
        "warm_renoise_one": ({}, (True, False), None),
        "warm_renoise_rows": ({}, (True, True), None),
        "warm_resume_one": ({}, (False, False), None),
        "warm_resume_rows": ({}, (False, True), None),
        "unguided": (dict(t_stop=T - STEPS), None, "unguided"),
        "unconditioned": (dict(t_stop=T - STEPS, condition=False), None, "no pairs"),
        "keep_row0": (dict(zero_row0=False), (True, False), None),  # (reaches t == 1)
        "device_result": (dict(t_stop=T - STEPS, return_device=True), None, None),
        "warm_device_result": (dict(return_device=True), (True, True), None),
        "graph_twice": (dict(t_stop=T - STEPS), None, "graph"),
        "sharded": (dict(t_stop=T - STEPS), None, "allreduce"),  # (the single form's alone, explicit streams only)
        "full": ({}, None, None)}
FULL = ("host", "device_noise")  # the noise forms of the two whole-loop cells per form
ENTRY_POINTS = tuple(f"edmp_denoise_{k}{r}{s}_dev" for k in ("guided", "scenes") for r in ("", "_rng") for s in ("", "_segment")) + tuple(
    f"edmp_sampler_seed{k}{r}_dev" for k in ("", "_scenes") for r in ("", "_rng"))
#         name: (form, what is wrong)   - one per raise statement of the two methods, _prepare, _check_run and _check_warm
REFUSALS = {f"{form}:{what}": (form, what) for form, whats in (
    ("single", ("other_gpu", "guide_rows", "traj_len", "t_stop", "not_a_warm_start", "warm_string", "warm_allreduce", "t_start", "warm_t_stop", "x0_shape", "warm_noise_shape",
                "allreduce_numpy", "bad_string", "pinned_shape", "host_shape")),
    ("scenes", ("not_a_batch", "other_gpu", "traj_len", "t_stop", "not_a_warm_start", "warm_string", "t_start", "warm_t_stop", "x0_shape", "max_batch", "no_pairs", "string",
                "not_a_list", "pinned_mix", "stream_shape", "not_f64"))) for what in whats}


def cell_names():
    out = []
    for form in FORMS:
        for run, (_, _, extra) in RUNS.items():
            for noise in NOISES:
                if noise == "string" and (form == "scenes" or RUNS[run][1] is not None or extra == "allreduce"):
                    continue  # (refusals)
                if extra == "allreduce" and (form == "scenes" or noise in ("numpy", "device_noise")):
                    continue  # (refusals)
                if run == "full" and noise not in FULL:
                    continue
                out.append(f"{form}:{run}:{noise}")
    return out + list(REFUSALS)


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


class Spy:
    """stands in for a context's `lib`: forwards everything and notes every edmp_* entry point as it is called - of the loop's own
    (edmp_denoise_*, edmp_sampler_seed_*) also every integer argument and, for every pointer, whether it is null"""

    def __init__(self, lib):
        self.__dict__.update(lib=lib, calls=[])

    @staticmethod
    def _arg(a):
        if isinstance(a, (bool, int, np.integer)):
            return int(a)
        if a is None or (isinstance(a, C.c_void_p) and not a.value):
            return "null"
        return "ptr"

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("edmp_"):
            return fn

        def call(*args):
            self.calls.append([name] + [self._arg(a) for a in args[1:]] if name.startswith(("edmp_denoise_", "edmp_sampler_seed_")) else name)
            return fn(*args)
        return call


def run_lengths(calls):
    """the sequence as [call, repeats] runs"""
    out = []
    for c in calls:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return out


_RIG = None


def rig():
    """the objects every cell runs on, built once: two contexts (the device's own and its lane 1), the net on both, S guides and their batch"""
    global _RIG
    if _RIG is None:
        from edmp_amd import scenes
        from edmp_amd import weights as W
        from edmp_amd.diffusion import Diffusion
        from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch
        from edmp_amd.runtime import get_context, lane_context
        from edmp_amd.temporalunet import TemporalUNet

        base = get_context(DEV)
        r = dict(ctxs={"base": base, "lane1": lane_context(base, 1)}, cfgs=cfgs_for([1, 10], 3), sd=W.init_state_dict(5, 7, 32, TINY_DIMS))
        assert r["cfgs"]["total_batch_size"] == B
        r["net"] = TemporalUNet(None, 7, 32, base, dims=TINY_DIMS, state_dict=r["sd"], max_batch=S * B)
        r["net_lane1"] = TemporalUNet(None, 7, 32, r["ctxs"]["lane1"], dims=TINY_DIMS, state_dict=r["sd"], max_batch=S * B)
        r["guides"] = [IntersectionVolumeGuide(scenes.random_scene(100 + k, 4 + 3 * k), base, r["cfgs"], B) for k in range(S + 1)]
        r["batch"] = SceneBatch(r["guides"][:S])
        r["dif"] = Diffusion(T, base)
        sg = [scenes.random_start_goal(110 + k) for k in range(S)]
        r["starts"], r["goals"] = np.stack([a for a, _ in sg]), np.stack([b for _, b in sg])
        rs = np.random.RandomState(55)
        r["Z"] = [rs.standard_normal((T + 1, B) + CN) for _ in range(S)]
        r["x0"] = rs.standard_normal((S, B) + CN)
        _RIG = r
    return _RIG


def _noise(kind, streams, single):
    """`streams`: S host arrays (one for the single form) -> the noise= value of the form `kind`, and seed= where the form has one"""
    import torch

    from edmp_amd.diffusion import DeviceNoise, PinnedNoiseStream

    def one(z):
        if kind == "host":
            return z
        if kind == "device":
            return torch.tensor(z, device=DEV)
        pin = torch.from_numpy(z.copy()).pin_memory()
        if kind == "pinned":
            return pin
        assert kind == "stream", kind
        st = PinnedNoiseStream(pin)
        st.publish(pin.numel())
        return st

    if kind == "numpy":
        return dict(noise=None)
    if kind == "string":
        return dict(noise="device", seed=2**64 + 11)  # (taken modulo 2^64)
    if kind == "device_noise":
        return dict(noise=DeviceNoise(2**63 + 5) if single else DeviceNoise(seeds=[2**63 + 5, 0, 2**64 - 1][:len(streams)]))
    vals = [one(z) for z in streams]
    return dict(noise=vals[0] if single else vals)


def _call(form, noise_kw, kw, warm=None, unguided=False, pairs=True, Z=None, **over):
    """one call of the form's method on the rig -> what it returns"""
    from edmp_amd.diffusion import WarmStart

    r = rig()
    single = form == "single"
    Z = r["Z"] if Z is None else Z
    kw = dict(kw, chunk_steps=CHUNK)
    if warm is not None and not isinstance(warm, tuple):
        kw["warm_start"] = warm
    elif warm is not None:
        renoise, per_row = warm
        x0 = r["x0"] if per_row else r["x0"][:, 0]
        kw["warm_start"] = WarmStart(x0[0] if single else x0, STEPS, renoise=renoise)
        lo = 0 if renoise else 1
        Z = [z[lo:1 + STEPS] for z in Z]  # [eps][z of step 12] ... [z of step 1]
    kw.update(_noise(noise_kw, Z[:1] if single else Z, single) if isinstance(noise_kw, str) else noise_kw)
    kw.update(over)
    model = kw.pop("model", r["net"])
    cn = kw.pop("cn", CN)
    if single:
        guide = kw.pop("guide", None if unguided else r["guides"][0])
        sched = r["cfgs"]["guidance_schedule"] if guide is not None else None
        sg = dict(start=r["starts"][0], goal=r["goals"][0]) if pairs else {}
        return r["dif"].denoise_guided(model, guide, cn[1], cn[0], sched, **dict(dict(batch_size=B, **sg), **kw))
    if unguided:
        kw["guided"] = False
    batch = kw.pop("batch", r["batch"])
    starts, goals = (r["starts"], r["goals"]) if pairs else (None, None)
    return r["dif"].denoise_guided_scenes(model, batch, cn[1], cn[0], starts, goals, **kw)


def _refusal(form, what):
    """the call that the refusal `what` answers"""
    import torch

    from edmp_amd.diffusion import WarmStart
    from edmp_amd.guide import SceneBatch

    r = rig()
    single = form == "single"
    x0 = r["x0"][0, 0] if single else r["x0"][:, 0]
    ws = WarmStart(x0, STEPS)
    bad = lambda shape: [np.zeros(shape + (B,) + CN)] * S  # noqa: E731
    host, stop = "host", dict(t_stop=T - STEPS)
    case = {"other_gpu": lambda: _call(form, host, stop, model=r["net_lane1"]),
            "guide_rows": lambda: _call(form, host, stop, batch_size=B - 1),
            "traj_len": lambda: _call(form, host, stop, cn=(7, 48)),
            "t_stop": lambda: _call(form, host, dict(t_stop=T)),
            "not_a_warm_start": lambda: _call(form, host, {}, warm=x0),
            "warm_string": lambda: _call(form, dict(noise="device"), {}, warm=ws),
            "warm_allreduce": lambda: _call(form, host, {}, warm=(True, False), allreduce=lambda t: None),
            "t_start": lambda: _call(form, host, {}, warm=WarmStart(x0, T + 1)),
            "warm_t_stop": lambda: _call(form, host, dict(t_stop=STEPS), warm=ws),
            "x0_shape": lambda: _call(form, host, {}, warm=WarmStart(np.zeros((5,) + CN), STEPS)),
            "warm_noise_shape": lambda: _call(form, host, {}, warm=ws, Z=bad((STEPS,))),  # (the eps draw is missing)
            "allreduce_numpy": lambda: _call(form, "numpy", stop, allreduce=lambda t: None),
            "bad_string": lambda: _call(form, dict(noise="philox"), stop),
            "pinned_shape": lambda: _call(form, "pinned", stop, Z=bad((T,))),
            "host_shape": lambda: _call(form, host, stop, Z=bad((T,))),
            "not_a_batch": lambda: _call(form, host, stop, batch=r["guides"][0]),
            "max_batch": lambda: _call(form, dict(noise=r["Z"] + r["Z"][:1]), stop, batch=SceneBatch(r["guides"])),
            "no_pairs": lambda: _call(form, host, stop, pairs=False),
            "string": lambda: _call(form, dict(noise="device"), stop),
            "not_a_list": lambda: _call(form, dict(noise=r["Z"][0]), stop),
            "pinned_mix": lambda: _call(form, dict(noise=[torch.from_numpy(r["Z"][0].copy()).pin_memory()] + r["Z"][1:]), stop),
            "stream_shape": lambda: _call(form, host, stop, Z=bad((T,))),
            "not_f64": lambda: _call(form, dict(noise=[torch.from_numpy(z.astype(np.float32)) for z in r["Z"]]), stop)}[what]
    return case


def evaluate(name):
    """run the cell `name` -> its record"""
    import torch

    r = rig()
    spies = {k: Spy(c.lib) for k, c in r["ctxs"].items()}
    rec = {}
    np.random.seed(31)
    try:
        for k, c in r["ctxs"].items():
            c.lib = spies[k]
            c.sampler_T = c.bound_model = c.bound_guide = None  # (what is resident is asked for again: the calls do not depend on what the context ran before)
        if name in REFUSALS:
            try:
                _refusal(*REFUSALS[name])()
                rec["error"] = None
            except Exception as exc:  # noqa: BLE001  (the record holds whatever the parent raised)
                rec["error"] = [type(exc).__name__, str(exc)]
        else:
            form, run, noise = name.split(":")
            kw, warm, extra = RUNS[run]
            over, results = {}, []
            if extra == "allreduce":
                over["allreduce"] = lambda scalar: None  # (one rank: the sum over ranks is the scalar itself)
            if extra == "graph":
                r["dif"].set_graph_replay(True)
            try:
                for _ in range(2 if extra == "graph" else 1):
                    X = _call(form, noise, kw, warm, unguided=extra in ("unguided", "no pairs"), pairs=extra != "no pairs", **over)
                    device = isinstance(X, torch.Tensor)
                    results.append({"device": bool(device and X.is_cuda), "sha": sha(X.cpu().numpy() if device else X)})
            finally:
                if extra == "graph":
                    r["dif"].set_graph_replay(False)
            rec["results"] = results
            if extra == "allreduce":
                rec["hook"] = {k: r["dif"].hook_stats[k] for k in ("kind", "calls")}
    finally:
        for k, c in r["ctxs"].items():
            c.lib = spies[k].lib
    state = np.random.get_state()
    rec["random_state"] = [state[0], sha(state[1]), int(state[2]), int(state[3]), float(state[4]).hex()]
    rec["calls"] = {k: run_lengths(s.calls) for k, s in spies.items()}
    return json.loads(json.dumps(rec))
