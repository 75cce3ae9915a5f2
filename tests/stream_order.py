"""The stream discipline of docs/LAB_NOTES.md §3, made testable: every context runs on ONE non-default stream, device tensors of the
caller are adopted (Context.adopt: our stream waits for the caller's), tensors returned with return_device=True are handed over
(Context.hand_over: the caller's stream waits for ours).  A missing wait is a race that a test loses once in many runs; here the race
is made deterministic instead of repeated:

* `hold(stream)` occupies a stream for a bounded, calibrated time (torch.cuda._sleep; a chain of dependent matmuls where that is missing);
* `late(good, stream)` makes a device tensor that reads as poison (NaN, a sentinel for integers) until the hold in front of its copy ends -
  a call that adopts it computes on `good`, a call that does not computes on poison;
* `poison_free_blocks(ctx, like)` fills the blocks the caching allocator will hand out for the next call's outputs with poison, so that a
  result read before its kernel ran is poison and not an earlier call's correct answer;
* `TABLE` has one record per public entry point that takes or returns device tensors: how to call it on the smallest useful shape, which
  arguments may be device tensors, which results come back as device tensors, and which private workers it runs (`covers`).
  tests/test_stream_order_host.py holds the table against the package by `inspect`; tests/test_gpu_stream_order.py runs it.

The hold is derived from measured latency: 10 x the largest host time of one table call with ready inputs and no hold (the factor covers
host jitter on a shared machine), at least 20 ms, and never more than 250 ms in one hold.

The side stream of the tests is ONE stream per process, not a fresh one per case: torch hands `torch.cuda.Stream()` out of a fixed pool of
32 per device that wraps, so the 33rd fresh stream would be the context's own stream and every wait would hold trivially.  It is also
CHOSEN (side_stream): the runtime deals a process's streams over a few hardware queues, and a side stream that shares its queue with the
context's stream is serialised with it whatever the library does - measured on an MI355X: with the first fresh stream taken as it came,
Context.adopt and Context.hand_over patched out went unseen from the side stream and were seen from the default stream.

This module holds no fixtures and no hooks."""
import dataclasses
import functools
import time

import numpy as np
import torch

from edmp_amd import evaluation as EV

POISON_INT = -1234567
HOLD_FACTOR, HOLD_FLOOR_MS, HOLD_TARGET_CAP_MS, HOLD_CAP_MS = 10.0, 20.0, 200.0, 250.0  # (accepted band: target .. 1.25 target <= the cap)
CALIBRATION_STEPS = 8
T = 255
T_STOP = T - 6       # the loops of the table run six reverse steps (two of them guided): the stream order does not depend on the step count
WARM_T = 8           # a warm start's t_start
PERIOD_SAMPLES = 15.5

_state = {"holds": 0}   # per process: the calibration, the latencies, the count of holds enqueued


# ---- poison, hold, late ------------------------------------------------------------------------------------------------------------------
def poison_(t):
    """fill a device tensor with poison in place, on the current stream"""
    if t.is_floating_point():
        return t.fill_(float("nan"))
    if t.dtype == torch.bool:
        return t.fill_(True)
    return t.fill_(POISON_INT)


def _mm_operands():
    if "mm" not in _state:
        n = 2048
        _state["mm"] = (torch.eye(n, device="cuda").roll(1, 0), torch.randn(n, n, device="cuda"))  # a permutation: the chain's values stay as they are
    return _state["mm"]


def _enqueue(units):
    """the busy work of a hold on the current stream: `units` cycles of torch.cuda._sleep, or that many dependent matmuls"""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units))
    else:
        p, a = _mm_operands()
        for _ in range(int(units)):
            a = p @ a


def _time_units(units):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    _enqueue(units)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate(target_ms):
    """the unit count whose hold lasts target .. 1.25 target ms, found with two events in at most CALIBRATION_STEPS steps from a small start
    (each step scales towards the target from the last measurement, so no probe is aimed past it)"""
    assert 0 < target_ms <= HOLD_TARGET_CAP_MS
    sleep = hasattr(torch.cuda, "_sleep")
    if not sleep:
        _mm_operands()
        _time_units(1)  # (the library's first call)
    units, steps = (1_000_000 if sleep else 1), []
    for _ in range(CALIBRATION_STEPS):
        ms = _time_units(units)
        steps.append((int(units), round(ms, 3)))
        if target_ms <= ms <= 1.25 * target_ms:
            break
        units = max(1, int(units * min(1.1 * target_ms / max(ms, 1e-3), 64.0)))
    fit = [s for s in steps if 0.9 * target_ms <= s[1] <= HOLD_CAP_MS]  # (a clock that wanders between two probes: the best probe made serves)
    if not fit:
        raise RuntimeError(f"hold calibration did not settle: target {target_ms} ms, steps {steps}")
    units, ms = min(fit, key=lambda s: abs(s[1] - 1.1 * target_ms))
    _state.update(units=units, measured_hold_ms=ms, target_hold_ms=target_ms, kind="torch.cuda._sleep cycles" if sleep else "dependent 2048^2 matmuls",
                  calibration_steps=steps)
    return units


def hold(stream):
    """occupy `stream` for the calibrated time (calibration(): 10 x the largest measured call latency, at least 20 ms, at most 250 ms)"""
    if "units" not in _state:
        calibration()
    with torch.cuda.stream(stream):
        _enqueue(_state["units"])
        behind = torch.cuda.Event()
        behind.record(stream)
    _state["holds"] += 1
    return behind  # unsignalled while the hold lasts: behind.query() is False as long as what was enqueued meanwhile was enqueued in time


def ready(good, device):
    """a host array (or tensor) as a device tensor that has landed: made and synchronised beforehand"""
    t = good.to(device) if isinstance(good, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(good)).to(device)
    torch.cuda.synchronize()
    return t


def late_all(goods, stream, holds=1):
    """[late(g, stream) for g in goods] behind ONE hold (or `holds` of them in a row).  goods: device tensors that have landed (ready)"""
    with torch.cuda.stream(stream):
        out = [poison_(torch.empty_like(g)) for g in goods]
    stream.synchronize()  # the poison has landed: a call that does not wait reads poison, not what the block held before
    for _ in range(holds):
        _state["late_behind"] = hold(stream)  # (the event behind the last hold: see call_with_late_arguments)
    with torch.cuda.stream(stream):
        for o, g in zip(out, goods):
            o.copy_(g, non_blocking=True)
    return out


def late(good, stream, holds=1):
    """a device tensor of `good`'s shape and dtype, made on `stream`: poison, then a hold, then the copy of `good` - until the hold ends it
    reads as poison, anything ordered after `stream` sees `good`"""
    g = good if isinstance(good, torch.Tensor) and good.is_cuda else ready(good, torch.cuda.current_device())
    return late_all([g], stream, holds)[0]


def _block_class(nbytes):
    """the size the caching allocator rounds a request to: multiples of 512 bytes (of 2 MiB from 10 MiB on)"""
    step = 512 if nbytes < (10 << 20) else (2 << 20)
    return max(step, -(-int(nbytes) // step) * step)


def poison_free_blocks(ctx, like, copies=4, stream=None):
    """allocate blocks of the sizes of the allocations behind `like` (tensors - views count once, by their storage - or byte counts) under
    ctx.stream (or `stream`: a caller's), fill them with poison and drop them: the blocks that the allocator recycles for the next call's
    outputs then hold poison.  Counted per allocation class (_block_class): as many blocks as `like` has allocations in the class - what
    the call keeps alive at once - plus `copies` for the temporaries it frees on the way.  The poison is all-ones bytes here: NaN in
    every float format, -1 in every integer format.  (The caller keeps the reference results of its case alive meanwhile, so THEIR blocks
    cannot be handed out.)"""
    stream = ctx.stream if stream is None else stream
    sizes = list({t.untyped_storage().data_ptr(): t.untyped_storage().nbytes() for t in like if isinstance(t, torch.Tensor)}.values())
    sizes += [int(n) for n in like if not isinstance(n, torch.Tensor)]
    classes = {}
    for n in sizes:
        if n:
            classes[_block_class(n)] = classes.get(_block_class(n), 0) + 1
    with torch.cuda.stream(stream):
        junk = [torch.empty(n, dtype=torch.uint8, device=ctx.device).fill_(255) for n, count in classes.items() for _ in range(count + copies)]
    stream.synchronize()
    del junk


# ---- trees of arguments and results ------------------------------------------------------------------------------------------------------
def tree_get(tree, path):
    for k in path:
        tree = tree[k]
    return tree


def tree_set(tree, path, v):
    """a copy of `tree` (dicts and lists copied along the path only) with the leaf at `path` replaced"""
    if not path:
        return v
    c = dict(tree) if isinstance(tree, dict) else list(tree)
    c[path[0]] = tree_set(tree[path[0]], path[1:], v)
    return c


def flatten(res, prefix=""):
    """a result - dict, tuple, list, array, tensor, scalar or None - as {path: leaf}"""
    if isinstance(res, dict):
        items = res.items()
    elif isinstance(res, (tuple, list)):
        items = enumerate(res)
    else:
        return {prefix: res}
    out = {}
    for k, v in items:
        out.update(flatten(v, f"{prefix}.{k}" if prefix else str(k)))
    return out


def device_leaves(res):
    return {k: v for k, v in flatten(res).items() if isinstance(v, torch.Tensor) and v.is_cuda}


def host_leaf(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return v


def same_bits(a, b):
    """two leaves are equal bit for bit, NaN patterns included (arrays: dtype, shape and bytes)"""
    a, b = host_leaf(a), host_leaf(b)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)):
            a, b = np.asarray(a), np.asarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def differences(got, want):
    """the paths at which two results differ (a missing path differs)"""
    g, w = flatten(got), flatten(want)
    return sorted(k for k in set(g) | set(w) if k not in g or k not in w or not same_bits(g[k], w[k]))


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Call:
    """one call of an entry on host values: fn(**kwargs).  slots: {name: path into kwargs} of every argument that may be a device tensor;
    wrap: {top-level kwarg: f} applied after the slots were filled (a WarmStart around its x0); host_kwargs: where the host form of the call
    differs from the device form, the host form's arguments; before: run in front of every call (a seed of the global stream)"""

    fn: object
    kwargs: dict
    slots: dict
    wrap: dict = dataclasses.field(default_factory=dict)
    host_kwargs: dict = None
    before: object = None

    def run(self, values=None, return_device=None, host=False):
        """the call with the slots in `values` ({name: tensor}) replaced; the others stay host arrays"""
        kw = dict(self.host_kwargs) if (host and self.host_kwargs is not None) else dict(self.kwargs)
        for name, v in (values or {}).items():
            kw = tree_set(kw, self.slots[name], v)
        for k, f in self.wrap.items():
            kw[k] = f(kw[k])
        if return_device is not None:
            kw["return_device"] = return_device
        if self.before is not None:
            self.before()
        return self.fn(**kw)

    def goods(self):
        return {name: tree_get(self.kwargs, path) for name, path in self.slots.items()}


@dataclasses.dataclass(frozen=True)
class Entry:
    name: str                   # the case id
    target: str                 # module.qualname under edmp_amd of the public callable
    build: object               # rig -> Call
    device_args: tuple = ()     # the slots: arguments that may be device tensors
    device_results: tuple = ()  # with return_device: the result paths that are device tensors ("" = the result itself); empty: no return_device
    covers: tuple = ()          # the private workers (and helpers that test .is_cuda) the call runs, as module.qualname
    in_flight: bool = False     # the driver runs it on lane contexts (scenes_in_flight)

    @property
    def return_device(self):
        return bool(self.device_results)


def _walk(seed, n, N):
    from tests import timing_inputs as TI

    return np.ascontiguousarray(TI.walk_rows(seed, n, N, step=0.05))


class Rig:
    """what the table's calls share on one context: a guide over 4 obstacles (one a cylinder) with 4 plain rows, a 2 x 2 SceneBatch, the tiny
    net, a diffuser, and the host inputs - 4 rows of N = 8 waypoints (the metrics kernel's floor is N = 3: any N >= 3 runs every row kernel's
    real path), their profiles as the library itself gave them on host arrays, noise for six reverse steps, 2 IK targets x 8 seeds"""

    N = 8

    def __init__(self, ctx):
        self.ctx = ctx

    @functools.cached_property
    def cases(self):
        from tests import sdf_reference as R

        return [R.make_case(31 + s, 4, 12, 4, 1) for s in range(3)]

    def _guide(self, case, n, **kw):
        from edmp_amd import franka
        from edmp_amd.guide import IntersectionVolumeGuide
        from tests import ik_inputs, repair_inputs as RI

        cfgs = RI.plain_cfgs(n)
        g = IntersectionVolumeGuide(case["obstacle_config"], self.ctx, cfgs, cfgs["total_batch_size"], link_mesh_extents=franka.PLACEHOLDER_LINK_EXTENTS,
                                    obstacle_kinds=case["kinds"], goal_target=ik_inputs.fk(case["goal"]), **kw)
        return g, cfgs

    @functools.cached_property
    def _guide_cfgs(self):
        return self._guide(self.cases[0], 4)

    guide = property(lambda self: self._guide_cfgs[0])
    cfgs = property(lambda self: self._guide_cfgs[1])

    @functools.cached_property
    def batch(self):
        from edmp_amd.guide import SceneBatch

        return SceneBatch([self._guide(self.cases[1 + s], 2, bind=False)[0] for s in range(2)])

    @functools.cached_property
    def net(self):
        from tests.sdf_gpu import tiny_unet

        return tiny_unet(self.ctx)

    @functools.cached_property
    def dif(self):
        from edmp_amd.diffusion import Diffusion

        return Diffusion(T, self.ctx)

    # the pairs
    start = property(lambda self: self.cases[0]["start"])
    goal = property(lambda self: self.cases[0]["goal"])
    starts = property(lambda self: np.stack([self.cases[1 + s]["start"] for s in range(2)]))
    goals = property(lambda self: np.stack([self.cases[1 + s]["goal"] for s in range(2)]))

    @functools.cached_property
    def X(self):
        return _walk(5, 4, self.N)

    @functools.cached_property
    def XS(self):
        return _walk(6, 4, self.N).reshape(2, 2, 7, self.N)

    @functools.cached_property
    def Xint(self):
        """interior waypoints (4, 7, 6) as the cost and SDF reports of a guide take them"""
        return np.ascontiguousarray(self.X[:, :, 1:-1])

    def rows(self, owner):
        return self.X if owner == "guide" else self.XS

    def obj(self, owner):
        return self.guide if owner == "guide" else self.batch

    def pair(self, owner):
        return dict(start=self.start, goal=self.goal) if owner == "guide" else dict(starts=self.starts, goals=self.goals)

    @functools.lru_cache(maxsize=None)
    def profile(self, owner):
        return self.obj(owner).time_rows(self.rows(owner))

    @functools.lru_cache(maxsize=None)
    def beta(self, owner):
        return self.obj(owner).blend_rows(self.rows(owner))["beta"]

    @functools.lru_cache(maxsize=None)
    def blended_profile(self, owner):
        return self.obj(owner).time_blended_rows(self.rows(owner), self.beta(owner))

    def period(self, prof):
        d = np.nanmax(prof["duration"])
        return float(d) / PERIOD_SAMPLES if d > 0 else 1e-3

    @functools.cached_property
    def noise(self):
        return np.random.RandomState(9).standard_normal((T + 1, 4, 7, 50))

    @functools.cached_property
    def scene_noise(self):
        rs = np.random.RandomState(10)
        return [rs.standard_normal((T + 1, 2, 7, 50)) for _ in range(2)]

    @functools.cached_property
    def x0(self):
        """a prior plan per row: the line start -> goal"""
        t = np.linspace(0, 1, 50)
        return np.ascontiguousarray(np.broadcast_to(self.start[:, None] + t[None] * (self.goal - self.start)[:, None], (4, 7, 50)))

    @functools.cached_property
    def x0_scenes(self):
        t = np.linspace(0, 1, 50)
        return np.ascontiguousarray(self.starts[:, :, None] + t[None, None] * (self.goals - self.starts)[:, :, None])

    @functools.cached_property
    def candidates(self):
        """per scene its IK candidates (5 and 3, 7): the scene's goal and perturbations of it inside the limits"""
        from edmp_amd import franka

        lo, hi = franka.joint_limits()
        rs = np.random.RandomState(12)
        return [np.clip(self.goals[s][None] + 0.2 * rs.standard_normal((m, 7)), lo + 0.05, hi - 0.05) for s, m in enumerate((5, 3))]

    @functools.cached_property
    def ik_seeds(self):
        from edmp_amd import ik

        return ik.draw_seeds(8, 3)

    @functools.cached_property
    def ik_targets(self):
        """2 targets, each the pose of one of the 8 seeds every target is solved from: that seed is a solution at once"""
        from tests import ik_inputs

        return np.stack([ik_inputs.fk(self.ik_seeds[t]) for t in (1, 6)])


def _loop_kw(r, **kw):
    return dict(model=r.net, guide=r.guide, traj_len=50, num_channels=7, guidance_schedule=r.cfgs["guidance_schedule"], batch_size=4, start=r.start, goal=r.goal,
                t_stop=T_STOP, **kw)


def _scenes_kw(r, **kw):
    return dict(model=r.net, batch=r.batch, traj_len=50, num_channels=7, starts=r.starts, goals=r.goals, t_stop=T_STOP, **kw)


def _warm(x0_key, t_start):
    from edmp_amd.diffusion import WarmStart

    return {x0_key: lambda x0: WarmStart(x0, t_start, renoise=True)}


PROFILE_READ = ("y", "phase", "times", "duration", "seg")              # what edmp_sample_rows_dev reads of a profile
BLENDED_READ = ("beta",) + PROFILE_READ
G, E, D, K, U = "guide.IntersectionVolumeGuide", "evaluation", "diffusion.Diffusion", "ik", "temporalunet.TemporalUNet"
SB, SO = "guide.SceneBatch", "guide._SlotObject"
ROWS_F64 = (f"{SO}._rows_f64",)
STATE = (f"{SB}._state",) + ROWS_F64


def _rows_entries():
    """the finishing stages, on a guide, on a SceneBatch and as the functions of evaluation"""
    out = []

    def add(name, target, build, args, results=(), covers=(), in_flight=False):
        out.append(Entry(name, target, build, tuple(args), tuple(results), tuple(covers), in_flight))

    profile_slots = {f"profile.{k}": ("profile", k) for k in PROFILE_READ}
    blended_slots = {f"profile.{k}": ("profile", k) for k in BLENDED_READ}
    X = {"trajectories": ("trajectories",)}
    METRICS = ("joint_path_length", "ee_path_length", "joint_sparc", "ee_sparc")
    PROFILE = ("y", "phase", "times", "duration", "limit", "seg")
    SAMPLES = ("q", "qd", "count")
    for owner, cls, own in (("guide", G, ROWS_F64), ("scenes", SB, STATE)):
        p = "" if owner == "guide" else "scenes_"
        fl = owner == "guide"  # (the lane test runs the guide's stages)

        def rows(method, extra=lambda r, o: {}, slots=X, owner=owner):
            def build(r):
                return Call(getattr(r.obj(owner), method), dict(trajectories=r.rows(owner), **extra(r, owner)), dict(slots))
            return build

        add(p + "repair_rows", f"{cls}.repair_rows", rows("repair_rows", lambda r, o: dict(iters=4, **r.pair(o))), X,
            ("trajectories", "iterations", "cost0", "cost", "clearance0", "clearance"), own + (f"{SO}._repair",), fl)
        add(p + "shortcut_rows", f"{cls}.shortcut_rows", rows("shortcut_rows"), X, ("trajectories", "accepted", "tested", "length0", "length", "spans"),
            own + (f"{SO}._shortcut",), fl)
        add(p + "success_rows", f"{cls}.success_rows", rows("success_rows"), X, ("ok", "first", "within", "collision_free"), own + (f"{SO}._success",), fl)
        add(p + "self_collision_rows", f"{cls}.self_collision_rows", rows("self_collision_rows"), X, ("first", "pair", "free"), own + (f"{SO}._self_collision",))
        add(p + "time_rows", f"{cls}.time_rows", rows("time_rows"), X, PROFILE, own + (f"{E}.time_rows_on", f"{E}._rows_state"), fl)
        add(p + "blend_rows", f"{cls}.blend_rows", rows("blend_rows"), X, ("beta", "code", "halved", "tested"), own + (f"{SO}._blend",), fl)
        add(p + "sample_rows", f"{cls}.sample_rows",
            rows("sample_rows", lambda r, o: dict(profile=r.profile(o), period=r.period(r.profile(o)), rows=[2, 0]), {**X, **profile_slots}),
            [*X, *profile_slots], SAMPLES, own + (f"{E}.sample_rows_on", f"{E}._sample_setup", f"{E}._sample_result", f"{E}._rows_state", f"{E}._device_f64"))
        add(p + "time_blended_rows", f"{cls}.time_blended_rows", rows("time_blended_rows", lambda r, o: dict(beta=r.beta(o)), {**X, "beta": ("beta",)}),
            [*X, "beta"], PROFILE + ("blend", "beta"), own + (f"{E}.time_blended_rows_on", f"{E}._rows_state", f"{E}._device_f64"))
        add(p + "sample_blended_rows", f"{cls}.sample_blended_rows",
            rows("sample_blended_rows", lambda r, o: dict(profile=r.blended_profile(o), period=r.period(r.blended_profile(o))), {**X, **blended_slots}),
            [*X, *blended_slots], SAMPLES, own + (f"{E}.sample_blended_rows_on", f"{E}._sample_setup", f"{E}._sample_result", f"{E}._rows_state", f"{E}._device_f64"))
    add("metrics_rows", f"{G}.metrics_rows", lambda r: Call(r.guide.metrics_rows, dict(trajectories=r.X), dict(X)), X, METRICS, (f"{E}.metrics_rows_on",), True)

    # the functions of evaluation: `_on` takes the context, the other its device (a Context passes through get_context)
    def ev(fn, extra=lambda r: {}, slots=X):
        def build(r):
            f = getattr(EV, fn)
            return Call(functools.partial(f, r.ctx) if fn.endswith("_on") else functools.partial(f, device=r.ctx), dict(trajectories=r.X, **extra(r)), dict(slots))
        return build

    sampler = (f"{E}._sample_setup", f"{E}._sample_result", f"{E}._rows_state", f"{E}._device_f64")
    for s in ("_on", ""):
        fn = "metrics_rows_on" if s else "batch_metrics"
        add(fn, f"{E}.{fn}", ev(fn), X, METRICS, (f"{E}.metrics_rows_on",))
        add("ev_time_rows" + s, f"{E}.time_rows{s}", ev("time_rows" + s), X, PROFILE, (f"{E}.time_rows_on", f"{E}._rows_state"))
        add("ev_sample_rows" + s, f"{E}.sample_rows{s}",
            ev("sample_rows" + s, lambda r: dict(profile=r.profile("guide"), period=r.period(r.profile("guide"))), {**X, **profile_slots}), [*X, *profile_slots],
            SAMPLES, (f"{E}.sample_rows_on",) + sampler)
        add("ev_time_blended_rows" + s, f"{E}.time_blended_rows{s}", ev("time_blended_rows" + s, lambda r: dict(beta=r.beta("guide")), {**X, "beta": ("beta",)}),
            [*X, "beta"], PROFILE + ("blend", "beta"), (f"{E}.time_blended_rows_on", f"{E}._rows_state", f"{E}._device_f64"))
        add("ev_sample_blended_rows" + s, f"{E}.sample_blended_rows{s}",
            ev("sample_blended_rows" + s, lambda r: dict(profile=r.blended_profile("guide"), period=r.period(r.blended_profile("guide"))), {**X, **blended_slots}),
            [*X, *blended_slots], SAMPLES, (f"{E}.sample_blended_rows_on",) + sampler)
    return out


def _host_result_entries():
    """calls that accept device tensors and return host values (or a synchronised device tensor)"""
    out = []

    def add(name, target, build, args, covers=()):
        out.append(Entry(name, target, build, tuple(args), (), tuple(covers)))

    X = {"trajectories": ("trajectories",)}
    J = {"joint_tensor": ("joint_tensor",)}
    add("cost", f"{G}.cost", lambda r: Call(r.guide.cost, dict(joint_tensor=r.Xint.astype(np.float32), t=0), dict(J)), J, (f"{G}._cost_common",))
    add("swept_volume_cost", f"{G}.swept_volume_cost",
        lambda r: Call(r.guide.swept_volume_cost, dict(joint_tensor=r.Xint.astype(np.float32), start=r.start, goal=r.goal, t=0), dict(J)), J, (f"{G}._cost_common",))
    add("sdf_rows", f"{G}.sdf_rows", lambda r: Call(r.guide.sdf_rows, dict(trajectories=r.Xint, start=r.start, goal=r.goal), dict(X)), X, ROWS_F64 + (f"{SO}._sdf_report",))
    add("sdf_self_rows", f"{G}.sdf_self_rows", lambda r: Call(r.guide.sdf_self_rows, dict(trajectories=r.Xint), dict(X)), X, ROWS_F64 + (f"{SO}._self_report",))
    add("sdf_goal_rows", f"{G}.sdf_goal_rows", lambda r: Call(r.guide.sdf_goal_rows, dict(trajectories=r.Xint), dict(X)), X, ROWS_F64 + (f"{SO}._goal_report",))
    add("sdf_sweep_rows", f"{G}.sdf_sweep_rows", lambda r: Call(r.guide.sdf_sweep_rows, dict(trajectories=r.Xint, start=r.start, goal=r.goal, substeps=4), dict(X)), X,
        ROWS_F64 + (f"{SO}._sweep_report",))
    add("row_swept_volumes", f"{G}.row_swept_volumes", lambda r: Call(r.guide.row_swept_volumes, dict(trajectories=r.X, start=r.start, goal=r.goal), dict(X)), X,
        ROWS_F64 + (f"{SO}._swept",))
    for prefer in ("fastest", "shortest"):
        add(f"select_row_{prefer}", f"{G}.select_row",
            lambda r, prefer=prefer: Call(r.guide.select_row, dict(trajectories=r.X, start=r.start, goal=r.goal, prefer=prefer), dict(X)), X,
            ROWS_F64 + (f"{SO}._swept", f"{SO}._pick", f"{E}.metrics_rows_on", f"{E}.time_rows_on", f"{E}._rows_state"))
    add("choose_best_trajectory", f"{G}.choose_best_trajectory",
        lambda r: Call(r.guide.choose_best_trajectory, dict(trajectories=r.X, start=r.start, goal=r.goal, prefer="smoothest"), dict(X)), X, (f"{G}.select_row", f"{SO}._pick"))
    add("success_rate", f"{E}.success_rate", lambda r: Call(EV.success_rate, dict(trajectories=r.X, guide=r.guide), dict(X)), X,
        (f"{G}.success_rows",))
    add("self_collision_rate", f"{E}.self_collision_rate",
        lambda r: Call(EV.self_collision_rate, dict(trajectories=r.XS, guide=r.batch), dict(X)), X, (f"{SB}.self_collision_rows",))

    # the scene batch
    def flat_goals(r):
        return np.ascontiguousarray(np.concatenate(r.candidates)), np.asarray([c.shape[0] for c in r.candidates], dtype=np.int32)

    add("filter_goals", f"{SB}.filter_goals",
        lambda r: Call(r.batch.filter_goals, dict(starts=r.starts, goals=flat_goals(r)[0], counts=flat_goals(r)[1]), {"goals": ("goals",)},
                       host_kwargs=dict(starts=r.starts, goals=r.candidates)), ("goals",), ("guide.goal_filter_device_inputs",))
    P = lambda r: dict(starts=r.starts, goals=r.goals)  # noqa: E731
    add("scenes_row_swept_volumes", f"{SB}.row_swept_volumes", lambda r: Call(r.batch.row_swept_volumes, dict(trajectories=r.XS, **P(r)), dict(X)), X,
        STATE + (f"{SB}._volumes", f"{SO}._swept"))
    add("scenes_select_rows", f"{SB}.select_rows", lambda r: Call(r.batch.select_rows, dict(trajectories=r.XS, prefer="fastest", **P(r)), dict(X)), X,
        STATE + (f"{SB}._volumes", f"{SO}._swept", f"{SO}._pick", f"{E}.metrics_rows_on", f"{E}.time_rows_on"))
    add("scenes_choose_best_trajectories", f"{SB}.choose_best_trajectories",
        lambda r: Call(r.batch.choose_best_trajectories, dict(trajectories=r.XS, prefer="shortest", **P(r)), dict(X)), X, (f"{SB}.select_rows", f"{SO}._pick"))
    add("scenes_sdf_rows", f"{SB}.sdf_rows", lambda r: Call(r.batch.sdf_rows, dict(trajectories=r.XS, **P(r)), dict(X)), X, STATE + (f"{SO}._sdf_report",))
    add("scenes_sdf_sweep_rows", f"{SB}.sdf_sweep_rows", lambda r: Call(r.batch.sdf_sweep_rows, dict(trajectories=r.XS, substeps=4, **P(r)), dict(X)), X,
        STATE + (f"{SO}._sweep_report",))
    add("scenes_sdf_self_rows", f"{SB}.sdf_self_rows", lambda r: Call(r.batch.sdf_self_rows, dict(trajectories=r.XS), dict(X)), X, STATE + (f"{SO}._self_report",))
    add("scenes_sdf_goal_rows", f"{SB}.sdf_goal_rows", lambda r: Call(r.batch.sdf_goal_rows, dict(trajectories=r.XS), dict(X)), X, STATE + (f"{SO}._goal_report",))

    # the network and the single reverse step
    add("unet_forward", f"{U}.forward",
        lambda r: Call(r.net.forward, dict(x=np.random.RandomState(3).standard_normal((4, 7, 50)).astype(np.float32), t=100), {"x": ("x",)}), ("x",))
    add("p_sample_using_posterior", f"{D}.p_sample_using_posterior",
        lambda r: Call(r.dif.p_sample_using_posterior, dict(xt=r.x0, t=100, eps=np.random.RandomState(4).standard_normal((4, 7, 50)).astype(np.float32),
                                                            z=np.random.RandomState(5).standard_normal((4, 7, 50))), {"eps": ("eps",)}), ("eps",))
    return out


def _loop_entries():
    """the two denoise loops from every noise source, and IK"""
    out = []

    def add(name, target, build, args, results=("",), covers=(), in_flight=False):
        out.append(Entry(name, target, build, tuple(args), tuple(results), tuple(covers), in_flight))

    run = (f"{D}._run", f"{D}._finish", "diffusion._is_pinned_f64")
    add("denoise_guided", f"{D}.denoise_guided", lambda r: Call(r.dif.denoise_guided, _loop_kw(r, noise=r.noise), {"noise": ("noise",)}), ("noise",), covers=run, in_flight=True)
    add("denoise_guided_warm", f"{D}.denoise_guided",
        lambda r: Call(r.dif.denoise_guided, {**_loop_kw(r, noise=r.noise[:1 + WARM_T], warm_start=r.x0), "t_stop": 0}, {"noise": ("noise",), "x0": ("warm_start",)},
                       wrap=_warm("warm_start", WARM_T)), ("noise", "x0"), covers=run)

    def device_noise(r):
        from edmp_amd.diffusion import DeviceNoise

        return Call(r.dif.denoise_guided, _loop_kw(r, noise=DeviceNoise(11)), {})

    add("denoise_guided_device_noise", f"{D}.denoise_guided", device_noise, (), covers=run)

    def numpy_stream(r):
        return Call(r.dif.denoise_guided, _loop_kw(r), {}, before=lambda: np.random.seed(17))

    add("denoise_guided_numpy_stream", f"{D}.denoise_guided", numpy_stream, (), covers=run + (f"{D}._run_numpy_stream", f"{D}._run_segments"))
    add("denoise_guided_pinned", f"{D}.denoise_guided", lambda r: Call(r.dif.denoise_guided, _loop_kw(r, noise=torch.from_numpy(r.noise).pin_memory()), {}), (),
        covers=run + (f"{D}._pinned_chunks", f"{D}._run_segments"))
    pieces = {"noise[0]": ("noise", 0), "noise[1]": ("noise", 1)}
    add("denoise_guided_scenes", f"{D}.denoise_guided_scenes", lambda r: Call(r.dif.denoise_guided_scenes, _scenes_kw(r, noise=list(r.scene_noise)), dict(pieces)),
        tuple(pieces), covers=run + ("diffusion.place_scene_rows",))
    add("denoise_guided_scenes_warm", f"{D}.denoise_guided_scenes",
        lambda r: Call(r.dif.denoise_guided_scenes, {**_scenes_kw(r, noise=[z[:1 + WARM_T] for z in r.scene_noise], warm_start=r.x0_scenes), "t_stop": 0},
                       {**pieces, "x0": ("warm_start",)}, wrap=_warm("warm_start", WARM_T)), (*pieces, "x0"), covers=run)

    def solve(r):
        from edmp_amd import ik

        return Call(functools.partial(ik.solve, r.ctx), dict(targets=r.ik_targets, seeds=[r.ik_seeds, r.ik_seeds], return_all=True), {})

    def solve_many(r):
        from edmp_amd import ik

        return Call(ik.FrankaIK(r.ctx, n_seeds=8, seed=3).solve_many, dict(targets=r.ik_targets), {})

    add("ik_solve", f"{K}.solve", solve, (), ("goals", "q", "residuals", "valid"))
    add("ik_solve_many", f"{K}.FrankaIK.solve_many", solve_many, (), ("goals",), (f"{K}.solve",))
    return out


TABLE = tuple(_rows_entries() + _host_result_entries() + _loop_entries())
BY_NAME = {e.name: e for e in TABLE}
assert len(BY_NAME) == len(TABLE)


# ---- rigs, latencies, the calibrated hold -------------------------------------------------------------------------------------------------
_rigs = {}


def rig(which="base"):
    """the rig of the base context ("base") or of lane 1 of the same GPU ("lane1"), built once per process"""
    if which not in _rigs:
        from edmp_amd.runtime import get_context, lane_context
        from tests.sdf_gpu import DEV

        base = get_context(DEV)
        _rigs[which] = Rig(base if which == "base" else lane_context(base, 1))
    return _rigs[which]


@functools.lru_cache(maxsize=None)
def call_of(name, which="base"):
    return BY_NAME[name].build(rig(which))


def _blocked_ms(stream, others):
    """hold `stream`, then enqueue a trivial operation on each of `others`: the host time [ms] until each of those has run.  Streams that
    the runtime feeds through one hardware queue run in queue order, and the hold then delays a stream it was never ordered against."""
    evs = []
    torch.cuda.synchronize()
    hold(stream)
    t0 = time.perf_counter()
    for o in others:
        with torch.cuda.stream(o):
            torch.zeros(1, device="cuda")
            ev = torch.cuda.Event()
            ev.record(o)
        evs.append(ev)
    out = []
    for ev in evs:
        ev.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    torch.cuda.synchronize()
    return out


def side_stream():
    """the one side stream of the process (see the module docstring): a torch stream that is none of the contexts' own AND that the runtime
    runs beside them - a process opens a handful of hardware queues and deals its streams over them, and two streams that share a queue are
    serialised by it: under a hold on such a side stream every wait would hold trivially.  Candidates are probed with one hold each until
    one leaves both contexts' streams running (the probes go into the record)."""
    if "side" not in _state:
        calibration()
        ctxs = [rig("base").ctx, rig("lane1").ctx]
        taken = {torch.cuda.default_stream().cuda_stream}
        for c in ctxs:
            taken.add(c.stream.cuda_stream)
            if hasattr(c, "copy_stream"):
                taken.add(c.copy_stream.cuda_stream)
        probes = _state.setdefault("side_stream_probes", [])
        for k in range(31):
            s = torch.cuda.Stream()
            if s.cuda_stream in taken:
                continue
            taken.add(s.cuda_stream)
            ms = _blocked_ms(s, [c.stream for c in ctxs])
            probes.append([k] + [round(v, 3) for v in ms])
            if max(ms) < 0.25 * _state["measured_hold_ms"]:
                _state["side"] = s
                break
        else:
            raise RuntimeError(f"every torch stream is serialised with a context's stream on this runtime: {probes}")
    return _state["side"]


def caller_stream(caller):
    return torch.cuda.default_stream() if caller == "default" else side_stream()


@functools.lru_cache(maxsize=None)
def host_result(name, which="base"):
    """the entry's result on host arrays: computed once, shared by the comparisons, left unchanged"""
    return call_of(name, which).run(host=True)


def device_inputs(call, device):
    """every slot of a call as a device tensor that has landed"""
    vals = {name: ready(g, device) for name, g in call.goods().items()}
    torch.cuda.synchronize()
    return vals


def calibration():
    """measured once per process: with ready inputs and no hold, the host time from entering each table entry's call to its return (the
    second call: the first binds, uploads tables and builds what is built lazily); the hold = 10 x the largest, at least 20 ms; its
    calibrated unit count.  Returns the record that goes to profiles/stream_order.json."""
    if "latency_ms" in _state:
        return _state
    r = rig("base")
    lat = {}
    for e in TABLE:
        call = call_of(e.name)
        vals = device_inputs(call, r.ctx.device)
        took = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call.run(vals)
            took.append(1e3 * (time.perf_counter() - t0))
        lat[e.name] = min(took[1:])  # (the smaller of two warm calls: one hiccup of the host is not the entry's latency)
    torch.cuda.synchronize()
    worst = max(lat.values())
    target = max(HOLD_FACTOR * worst, HOLD_FLOOR_MS)
    assert HOLD_FACTOR * worst <= HOLD_TARGET_CAP_MS, (f"{HOLD_FACTOR:g} x the largest call latency ({worst:.1f} ms: {max(lat, key=lat.get)}) is more than one hold may "
                                                       f"last ({HOLD_TARGET_CAP_MS:g} ms): a shorter hold would not cover host jitter - make that entry's call smaller")
    _state.update(latency_ms={k: round(v, 3) for k, v in lat.items()}, largest_latency_ms=round(worst, 3), hold_factor=HOLD_FACTOR)
    calibrate(target)
    return _state


# ---- the two comparisons ------------------------------------------------------------------------------------------------------------------
ATTEMPTS = 3  # of a case whose premise did not hold (the host was paused past the hold): such an attempt decides nothing and is discarded


def call_with_late_arguments(entry, caller, which="base", only=None):
    """the entry's result with its device arguments made `late` on the caller's stream (`only`: that one slot late, the others host arrays)
    -> (result, decided).  decided: the case's premise held - when the library first adopted one of the late arguments (Context.adopt, or
    whatever a test put in its place, is wrapped for the call to note it) the hold in front of their copies was still running, so a read
    without the wait would have met poison.  Not decided: the host was paused past the hold (or nothing late was ever adopted)."""
    from edmp_amd.runtime import Context

    call, ctx = call_of(entry.name, which), rig(which).ctx
    calibration()
    slots = [only] if only is not None else list(call.slots)
    goods = [ready(call.goods()[s], ctx.device) for s in slots]
    stream = caller_stream(caller)
    inner, noted = Context.adopt, []
    with torch.cuda.stream(stream):
        lates = late_all(goods, stream)
        behind, ptrs = _state["late_behind"], {t.data_ptr() for t in lates}

        def noting(self, t):
            if t.data_ptr() in ptrs:
                noted.append(behind.query())
            return inner(self, t)

        Context.adopt = noting
        try:
            got = call.run(dict(zip(slots, lates)))
        finally:
            Context.adopt = inner
    torch.cuda.synchronize()
    return got, bool(noted) and not noted[0]


def adoption_differences(entry, caller, which="base", only=None):
    """call_with_late_arguments against the same call on host arrays made beforehand -> (the result paths that differ - none: every late
    argument was adopted before it was read -, decided)"""
    got, decided = call_with_late_arguments(entry, caller, which, only)
    return differences(got, host_result(entry.name, which)), decided


def hand_over_differences(entry, caller, which="base"):
    """the mirror image: our stream held, the entry called with device inputs and return_device=True, every returned device tensor cloned
    and every device input overwritten with poison on the caller's stream at once, without a synchronisation -> (the result paths whose clone
    differs from the unheld call's result, the paths that came back as device tensors, decided).  decided: the hold on our stream was still
    running when the clones and the overwrites had been enqueued.  An entry that synchronises with the host before it returns can never
    be decided this way: it sits out the hold, and its results are ordered by that synchronisation."""
    call, ctx = call_of(entry.name, which), rig(which).ctx
    calibration()
    ref = call.run(device_inputs(call, ctx.device), return_device=True)   # kept alive until the case ends
    torch.cuda.synchronize()
    want = {k: host_leaf(v) for k, v in flatten(ref).items()}
    vals = device_inputs(call, ctx.device)
    stream = caller_stream(caller)
    poison_free_blocks(ctx, list(device_leaves(ref).values()))
    torch.cuda.synchronize()
    behind = hold(ctx.stream)
    with torch.cuda.stream(stream):
        got = call.run(vals, return_device=True)
        flat = flatten(got)
        clones = {k: (v.clone() if isinstance(v, torch.Tensor) and v.is_cuda else v) for k, v in flat.items()}
        for v in vals.values():
            poison_(v)  # write after read: our kernel may still be reading the input
    decided = not behind.query()
    torch.cuda.synchronize()
    bad = sorted(k for k in set(clones) | set(want) if k not in clones or k not in want or not same_bits(clones[k], want[k]))
    del ref
    return bad, sorted(device_leaves(got)), decided
