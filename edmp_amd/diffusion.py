"""Diffusion — host-side mirror of the reference sampler object (diffusion/diffusion.py:8-356).  The reverse loop
(`denoise_guided`) runs device-resident in libedmp_hip.so (edmp_amd/csrc/sampler.hip): one host call per scene."""
from __future__ import annotations

import contextlib
import ctypes as C
import operator
import os
import threading
import time
from typing import NamedTuple

import numpy as np
import torch

from . import _capi, franka, nprng
from .runtime import get_context, ptr


def draw_noise(T: int, batch_size: int, num_channels: int, traj_len: int) -> np.ndarray:
    """(T+1, B, C, N) f64 from the GLOBAL NumPy RandomState in the reference's call order: one
    ``multivariate_normal(0, I_N, size=(B, C))`` for X_T (diffusion.py:303) then one per step (diffusion.py:126).
    With an identity covariance that call consumes the stream exactly like ``standard_normal((B, C, N))``
    (pinned by tests/test_host.py), so all draws are made in one vectorised call - by edmp_amd.nprng, which produces
    NumPy's legacy stream bit for bit on all host cores and advances the global state exactly like NumPy."""
    return nprng.standard_normal((T + 1, batch_size, num_channels, traj_len))


def _startgoal(start, goal, needed: bool):
    """(7,) f64 start / goal for the C ABI (which reads 7 doubles from each).  The reference allows None when it neither
    conditions nor guides (diffusion.py:253, 300): zeros stand in there; anything else must have exactly 7 entries."""
    out = []
    for name, v in (("start", start), ("goal", goal)):
        if v is None:
            if needed:
                raise ValueError(f"{name} is required when conditioning or guiding")
            v = np.zeros(7)
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
        if a.size != 7:
            raise ValueError(f"{name} must have 7 joint values, got shape {np.shape(v)}")
        out.append(a)
    return out


DEFAULT_CHUNK_STEPS = 16


class Segment(NamedTuple):
    """one piece of a run whose noise arrives in chunks: reverse steps t_hi .. t_lo + 1, under `draws` draws of (B, C, N) that begin
    `offset` draws into the run's stream; `init`: the first piece, whose chunk begins with X_T"""

    t_hi: int
    t_lo: int
    init: bool
    draws: int
    offset: int


def chunk_plan(T, t_stop=0, chunk_steps=DEFAULT_CHUNK_STEPS):
    """The segments of a run from T down to t_stop.  The first chunks are short and double (1, 2, 4, ... steps, capped at
    `chunk_steps`) so that the GPU starts after ONE step's worth of draws and the host gets ahead of it geometrically; X_T rides
    with the first chunk.  Every producer and consumer of chunked noise (the draw thread, the pinned uploads, infer_serial's feeder
    and its watermarks) works in units of this plan."""
    plan, t_hi, k, offset = [], int(T), 1, 0
    while t_hi > int(t_stop):
        steps = min(k, int(chunk_steps), t_hi - int(t_stop))
        seg = Segment(t_hi, t_hi - steps, not plan, steps + (0 if plan else 1), offset)
        plan.append(seg)
        t_hi, k, offset = seg.t_lo, 2 * k, offset + seg.draws
    return plan


def warm_plan(t_start, t_stop=0, lead=1, chunk_steps=DEFAULT_CHUNK_STEPS):
    """The segments of a warm-started run from t_start down to t_stop: chunk_plan's, whose first segment (`init`: the seed call comes
    first) carries `lead` extra draws in front of its steps' - 1 = the eps draw of the re-noising, which rides where X_T's draw rides in
    a full run; 0 = a resume, whose stream holds the steps' draws only."""
    if lead not in (0, 1):
        raise ValueError(f"lead must be 0 or 1, got {lead}")
    plan = chunk_plan(t_start, t_stop, chunk_steps)
    if lead:
        return plan
    return [Segment(s.t_hi, s.t_lo, s.init, s.draws - (1 if s.init else 0), s.offset - (0 if s.init else 1)) for s in plan]


class WarmStart:
    """A prior plan to start the reverse loop from at step `t_start` instead of from pure noise at T (`warm_start=` of
    Diffusion.denoise_guided / denoise_guided_scenes).  `x0`: host array or tensor, or device tensor, of real numbers: (C, N) - one plan
    for every row - or (B, C, N); for a scene batch (S, C, N) - one plan per scene - or (S, B, C, N).  `renoise`: forward-noise x0 to
    t_start with the first draw of the call's noise stream (q(x_t | x_0)); False takes x0 as the state at t_start itself, e.g. what a
    call with t_stop = t_start returned.  Whether the shape fits the run and t_start lies in 1..T is checked by the call that uses it."""

    def __init__(self, x0, t_start, renoise=True):
        if isinstance(t_start, bool):
            raise TypeError("t_start must be an integer, got a bool")
        try:
            self.t_start = operator.index(t_start)
        except TypeError:
            raise TypeError(f"t_start must be an integer, got {type(t_start).__name__}") from None
        if isinstance(x0, torch.Tensor):
            if x0.dtype == torch.bool or x0.is_complex():
                raise TypeError(f"x0 must hold real numbers, got {x0.dtype}")
        else:
            x0 = np.asarray(x0)
            if x0.dtype.kind not in "fiu":
                raise TypeError(f"x0 must hold real numbers, got dtype {x0.dtype}")
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.ndim not in (2, 3, 4) or 0 in tuple(x0.shape):
            raise ValueError(f"x0 must be (C, N) or (B, C, N) - scene batch: (S, C, N) or (S, B, C, N) -, got shape {tuple(x0.shape)}")
        self.x0 = x0
        self.renoise = bool(renoise)

    @property
    def lead(self) -> int:
        """draws in front of the steps' in the run's noise stream: the eps draw when re-noising"""
        return 1 if self.renoise else 0


class DeviceNoise:
    """The device noise source (Philox4x32-10 + Box-Muller inside the step tail, csrc/tail.h) as a ``noise=`` value, for every run form:
    ``DeviceNoise(seed)`` - one scene (Diffusion.denoise_guided / denoise) - or ``DeviceNoise(seeds=[...])`` - one seed per scene of a
    scene batch (Diffusion.denoise_guided_scenes).  Seeds are integers in [0, 2^64); equal seeds are allowed.  Row b, waypoint l of a
    scene draws Philox counter (b N + l, step, block, 0) under the scene's seed as key - the index is the scene's own, so a scene's numbers
    do not depend on its neighbours in a batch; step 0 = X_T of a full run or the eps of a re-noising warm start, 1 + T - t = reverse step
    t.  A full single-scene run is exactly ``noise="device", seed=seed``.  Nothing is drawn, page-locked or uploaded on the host."""

    def __init__(self, seed=None, *, seeds=None):
        if (seed is None) == (seeds is None):
            raise ValueError("DeviceNoise takes one seed, or seeds=[one per scene]")
        self.single = seeds is None
        vals = []
        for v in ([seed] if self.single else list(seeds)):
            if isinstance(v, bool):
                raise TypeError("a seed must be an integer, got a bool")
            try:
                v = operator.index(v)
            except TypeError:
                raise TypeError(f"a seed must be an integer, got {type(v).__name__}") from None
            if not 0 <= v < 2**64:
                raise ValueError(f"a seed must lie in [0, 2^64), got {v}")
            vals.append(v)
        if not vals:
            raise ValueError("DeviceNoise(seeds=...) needs at least one seed")
        self.seeds = tuple(vals)

    def _for_run(self, n_scenes, allreduce=None):
        """the seeds for a run of `n_scenes` scenes (None = a single-scene call), before anything is bound or enqueued"""
        if allreduce is not None:
            raise ValueError("the device noise source does not combine with a sharded run (allreduce=...): its element index is the row's "
                             "index on this rank")
        if n_scenes is None:
            if not self.single:
                raise ValueError("a single-scene run takes DeviceNoise(seed), not DeviceNoise(seeds=[...])")
            return self.seeds[0]
        if self.single:
            raise ValueError(f"a scene batch takes DeviceNoise(seeds=[...]) with one seed per scene ({n_scenes}), not a single seed")
        if len(self.seeds) != n_scenes:
            raise ValueError(f"DeviceNoise holds {len(self.seeds)} seeds, the scene batch has {n_scenes} scenes")
        return (C.c_uint64 * n_scenes)(*self.seeds)


def guided_step(t) -> bool:
    """the reverse steps that add the guide's gradient: every second one, down to t = 5 (diffusion.py:311, 326-327; the device loop's
    own copy of the rule is guided_step in csrc/sampler.hip)"""
    return (t % 2) < 1 and t >= 5


def _is_pinned_f64(x) -> bool:
    """a contiguous f64 tensor in page-locked host memory: what the copy stream can upload by DMA, slice by slice"""
    return isinstance(x, torch.Tensor) and not x.is_cuda and x.is_pinned() and x.dtype == torch.float64 and x.is_contiguous()


def _noise_error(name, want, x):
    return ValueError(f"{name} must be f64 {tuple(want)}, got {tuple(x.shape)} {x.dtype}")


def place_scene_rows(dst: torch.Tensor, pieces) -> torch.Tensor:
    """A scene batch's noise layout: ``pieces`` = S tensors (steps, B, C, N), scene s's draws; ``dst`` (steps, S*B, C, N) receives
    piece s at rows [s*B, (s+1)*B) of every draw, by one strided copy per scene (on the current stream)."""
    S = len(pieces)
    steps, SB = dst.shape[0], dst.shape[1]
    if S < 1 or SB % S:
        raise ValueError(f"{SB} rows do not split over {S} scenes")
    B = SB // S
    for s, p in enumerate(pieces):
        if tuple(p.shape) != (steps, B) + tuple(dst.shape[2:]):
            raise ValueError(f"scene {s}: piece {tuple(p.shape)} does not fit ({steps}, {B}) + {tuple(dst.shape[2:])}")
        dst[:, s * B:(s + 1) * B].copy_(p)
    return dst


class PinnedNoiseStream:
    """A (T+1, B, C, N) f64 noise stream in page-locked host memory that is still BEING DRAWN: the producer (infer_serial's feeder
    thread) fills it front to back and publishes how far it got; `Diffusion.denoise_guided(noise=stream)` uploads chunk after chunk as
    soon as each is complete - the first scene of a run starts after one step's worth of draws, later scenes find their stream ready."""

    def __init__(self, tensor):
        self.tensor, self.drawn, self.error = tensor, 0, None
        self._cv = threading.Condition()

    def publish(self, n_doubles, error=None):
        with self._cv:
            self.drawn, self.error = int(n_doubles), error
            self._cv.notify_all()

    def wait_until(self, n_doubles):
        with self._cv:
            while self.drawn < n_doubles and self.error is None:
                self._cv.wait()
            if self.error is not None:
                raise self.error


class _Form(NamedTuple):
    """what a single-scene run and a scene batch differ in once their arguments are checked (Diffusion._run).  The entry points are
    edmp_denoise_<kind>[_rng][_segment]_dev and edmp_sampler_seed[_scenes][_rng]_dev: _rng with `seeds`, _segment for a part of the loop."""

    kind: str        # "guided" | "scenes"
    lead: tuple      # the leading arguments of every call and the run's shape in front of (C, N): (B,) or (S, B)
    seeds: object    # the device source's seed (one scene) or (S) seeds as those entry points take them; None: the run reads noise streams
    place: object    # a scene batch: place(chunk (draws, S*B, C, N), S pieces (draws, B, C, N)) assembles a chunk of noise; None: one stream, its own chunk
    settle: bool     # a scene batch synchronises with the host where one scene does not: before a device result of any direct run is handed over,
                     # after a warm device-source run (its x0 upload may die), and before an error of a resident-stream run propagates


class Diffusion:
    """Same constructor / method signatures as the reference ``Diffusion(T, device, variance_thresh=0.02)``."""

    def __init__(self, T, device, variance_thresh=0.02):
        self.T = int(T)
        self.variance_thresh = float(variance_thresh)
        self.ctx = get_context(device)
        self.device = self.ctx.device
        self.ctx.ensure_sampler(self.T, self.variance_thresh)
        self.beta = np.zeros(self.T)
        self.alpha = np.zeros(self.T)
        self.alpha_bar = np.zeros(self.T)
        _capi.check(self.ctx.lib.edmp_sampler_read_schedule(self.ctx.h, _capi.as_pd(self.beta), _capi.as_pd(self.alpha), _capi.as_pd(self.alpha_bar)))

    def schedule_variance(self, thresh=0.02):
        return self.beta.copy()

    # ---- single pieces (reference API) ------------------------------------------------------------------------
    def p_sample_using_posterior(self, xt, t, eps, z=None):
        """diffusion.py:116-135.  Draws z from the global NumPy RNG like the reference unless ``z`` is given."""
        ctx = self.ctx
        ctx.ensure_sampler(self.T, self.variance_thresh)
        b, c, n = xt.shape
        if z is None:
            z = nprng.standard_normal((b, c, n))
        X = ctx.to_dev(np.array(xt, dtype=np.float64), torch.float64)  # a fresh device tensor: updated in place below
        e = ctx.to_dev(eps, torch.float32)
        zd = ctx.to_dev(np.asarray(z, dtype=np.float64), torch.float64)
        _capi.check(ctx.lib.edmp_psample_dev(ctx.h, ptr(X), ptr(e), ptr(zd), b, c, n, int(t), 1), "edmp_psample_dev")
        return ctx.to_host(X)

    # ---- forward process (training-side data generation) -------------------------------------------------------
    def _q(self, x, t, eps, cumulative, condition=False):
        ctx = self.ctx
        ctx.ensure_sampler(self.T, self.variance_thresh)
        x = np.ascontiguousarray(x, dtype=np.float64)
        b, c, n = x.shape
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t), (b,)), dtype=np.int32)
        if eps is None:  # diffusion.py:68-71 / 95-98: an identity-covariance multivariate normal == standard normal draws
            eps = nprng.standard_normal((b, c * n)).reshape(b, c, n)
        xd = ctx.to_dev(x, torch.float64)
        ed = ctx.to_dev(np.ascontiguousarray(eps, dtype=np.float64), torch.float64)
        xt = ctx.empty((b, c, n), torch.float64)
        mean = ctx.empty((b, c, n), torch.float64)
        _capi.check(ctx.lib.edmp_q_sample_dev(ctx.h, ptr(xd), ptr(ed), _capi.as_pi32(t), b, c, n, int(cumulative), int(bool(condition)), ptr(xt),
                                              ptr(mean)), "edmp_q_sample_dev")
        return ctx.to_host(xt), ctx.to_host(mean), t

    def q_sample(self, x, t, eps=None):
        """q(x_t | x_{t-1}) (diffusion.py:52-77): (xt, mean, var)."""
        xt, mean, t = self._q(x, t, eps, cumulative=0)
        return xt, mean, np.sqrt(1 - self.alpha[t - 1])

    def q_sample_from_x0(self, x0, t, eps=None):
        """q(x_t | x_0) (diffusion.py:79-105): (xt, mean, var), var of shape (b,1,1) like the reference."""
        xt, mean, t = self._q(x0, t, eps, cumulative=1)
        return xt, mean, np.sqrt(1 - self.alpha_bar[t - 1, np.newaxis, np.newaxis])

    def generate_q_sample(self, x0, time_steps=None, condition=True, return_type="tensor"):
        """Training pairs (diffusion.py:201-251): random timesteps + noise from the global NumPy RNG in the reference's
        order, diffusion and conditioning on the GPU.  Returns (X, Y, time_steps, means, vars)."""
        b, c, n = x0.shape
        if time_steps is None:
            time_steps = np.random.randint(1, self.T + 1, size=(b,))
        eps = nprng.standard_normal((b, c, n))  # == multivariate_normal(0, I_n, size=(b, c))   (diffusion.py:231)
        xt, means, t = self._q(x0, time_steps, eps, cumulative=1, condition=condition)
        vars_ = np.sqrt(1 - self.alpha_bar[t - 1, np.newaxis, np.newaxis])
        if return_type == "tensor":
            return torch.tensor(xt, dtype=torch.float32), torch.tensor(eps, dtype=torch.float32), torch.tensor(time_steps, dtype=torch.float32), means, vars_
        if return_type == "numpy":
            return xt, eps.copy(), time_steps, means, vars_
        raise ValueError('return_type must be "tensor" or "numpy"')  # the reference falls through to a NameError here

    def set_graph_replay(self, on: bool):
        """Capture the device-resident loop of denoise_guided into a hipGraph and replay it (see edmp_sampler_set_graph)."""
        self.ctx.ensure_sampler(self.T, self.variance_thresh)
        _capi.check(self.ctx.lib.edmp_sampler_set_graph(self.ctx.h, 1 if on else 0))

    def clip_joints(self, joints):
        lo, hi = franka.joint_limits()
        return np.clip(joints, lo[np.newaxis, :, np.newaxis], hi[np.newaxis, :, np.newaxis])

    # ---- the loop ----------------------------------------------------------------------------------------------
    def _prepare(self, model, guide, batch_size, guidance_schedule, condition=None):
        """bind the model and the guide object - a guide with its rows for `batch_size`, or a SceneBatch, whose rows are its own
        (batch_size None) - and set the conditioning switch (`condition` None: left as it is)"""
        ctx = self.ctx
        if model.ctx is not ctx or (guide is not None and guide.ctx is not ctx):
            raise _capi.EdmpError("model, guide and diffuser must live on the same GPU")
        ctx.ensure_sampler(self.T, self.variance_thresh)
        model._bind()
        if guide is not None:
            guide._bind()
            if batch_size is not None:
                if guide.batch_size != batch_size:
                    raise ValueError(f"guide was built for batch {guide.batch_size}, denoise_guided called with {batch_size}")
                guide._set_rows(guidance_schedule if guidance_schedule is not None else guide._sched)
        if condition is not None:
            _capi.check(ctx.lib.edmp_sampler_set_condition(ctx.h, 1 if condition else 0))

    def _check_run(self, model, traj_len, num_channels, t_stop):
        if int(traj_len) != model.horizon or int(num_channels) != model.input_dim:
            raise ValueError(f"traj_len/num_channels ({traj_len}, {num_channels}) do not match the model's ({model.horizon}, {model.input_dim})")
        if not 0 <= int(t_stop) < self.T:
            raise ValueError(f"t_stop must lie in [0, {self.T}), got {t_stop}")

    def _check_warm(self, ws, t_stop, noise, allreduce, shapes):
        """a warm start against the run it is given to, before anything is bound or enqueued.  `shapes`: {accepted x0 shape: x0_rows of
        the seed call}.  Returns x0_rows."""
        if not isinstance(ws, WarmStart):
            raise ValueError("warm_start must be a diffusion.WarmStart")
        if isinstance(noise, str):
            raise ValueError("a warm start takes NumPy-stream noise: the device noise mode (noise='device') has no segment form")
        if allreduce is not None:
            raise ValueError("a warm start of a sharded run (allreduce=...) is not supported")
        if not 1 <= ws.t_start <= self.T:
            raise ValueError(f"warm start: t_start must lie in 1..{self.T}, got {ws.t_start}")
        if not 0 <= int(t_stop) < ws.t_start:
            raise ValueError(f"warm start: t_stop must lie in [0, t_start = {ws.t_start}), got {t_stop}")
        if tuple(ws.x0.shape) not in shapes:
            raise ValueError(f"warm start: x0 must have one of the shapes {sorted(shapes, key=len)}, got {tuple(ws.x0.shape)}")
        return shapes[tuple(ws.x0.shape)]

    @staticmethod
    def _after_lead(zd, seg, ws, per_step):
        """(eps pointer or None, pointer to the first step's draw) inside a warm run's chunk `zd`"""
        if seg.init and ws.renoise:
            return ptr(zd), C.c_void_p(zd.data_ptr() + per_step * 8)
        return None, ptr(zd)

    def _finish(self, out, return_device, *, sync=False, hand_over=True):
        """the result as the caller asked for it: a fresh host copy, or the device tensor itself - after a host synchronisation (`sync`)
        and / or with torch's current stream ordered after the context's (`hand_over`)"""
        if not return_device:
            return self.ctx.to_host(out)
        if sync:
            self.ctx.sync()
        return self.ctx.hand_over(out) if hand_over else out

    @contextlib.contextmanager
    def _sharded(self, allreduce):
        """One logical batch across GPUs: this rank holds a row shard of a larger reference batch; the only cross-row coupling, the
        whole-batch sum(g^2) (lib/guide.py:629), is summed over ranks between the two halves of every guided step - INSIDE the
        device-resident loop: the library calls the hook once per guided step with the context's stream and the device scalar, the
        collective is ordered by the stream (no host round trip).  The hook is in place for the body and `hook_stats` is read after it."""
        from .dist import RcclAllReduce

        ctx = self.ctx
        if isinstance(allreduce, RcclAllReduce):
            # the hook is native code installed once on this context (csrc/rccl_hook.hip): nothing to install per call
            if allreduce.ctx is not ctx or not allreduce.attached():
                raise ValueError("this RcclAllReduce is not attached to the diffuser's context (or was closed)")
            kind = "native ncclAllReduce (csrc/rccl_hook.hip)"

            def install(on):  # (off again after the body: other runs of this context are not shards)
                _capi.check(ctx.lib.edmp_rccl_enable(ctx.h, 1 if on else 0), "edmp_rccl_enable")
        else:
            kind = "python callback (ctypes -> torch.distributed)"
            sumsq = self.sumsq_tensor()

            def _hook(_user, _stream, _ptr):
                try:
                    with torch.cuda.stream(ctx.stream):  # RCCL orders itself after the gradient kernels / before step_b
                        allreduce(sumsq)
                    return 0
                except Exception as exc:  # surfaced by the C side as EDMP_ERR_STATE
                    self._hook_error = exc
                    return 1

            cb = _capi.ALLREDUCE_FN(_hook)

            def install(on):
                _capi.check(ctx.lib.edmp_sampler_set_allreduce(ctx.h, C.cast(cb, C.c_void_p) if on else None, None))

        def read_stats():
            raw = (C.c_uint64 * 3)()
            _capi.check(ctx.lib.edmp_sampler_allreduce_stats(ctx.h, raw, 1))
            # host time inside the hook, measured by the library around each call (any hook): GIL + collective enqueue
            self.hook_stats = dict(calls=int(raw[0]), total_s=1e-9 * int(raw[1]), max_s=1e-9 * int(raw[2]), kind=kind)

        self._hook_error = None
        install(True)
        read_stats()
        try:
            yield
        except _capi.EdmpError:
            if self._hook_error is not None:
                raise self._hook_error
            raise
        finally:
            install(False)
            read_stats()

    def _run_segments(self, plan, source, segment, out, return_device, drain=lambda: None):
        """The segmented loop.  For every segment of `plan` (chunk_plan), `source(seg)` gives its noise chunk as a device tensor and
        `segment(chunk, seg, X_out)` enqueues its steps; X_out is `out` for the last segment and None before.  `drain()` waits for what
        the source still has in flight on the host."""
        keep = []  # every chunk stays allocated until the stream has consumed it
        try:
            for seg in plan:
                keep.append(source(seg))
                segment(keep[-1], seg, out if seg is plan[-1] else None)
        except BaseException:
            # leave nothing in flight that still reads the staging ring, a pinned stream or the chunk tensors: the draw thread finishes
            # its current chunk, the stream drains, then the error propagates
            for wait in (drain, self.ctx.sync):
                try:
                    wait()
                except Exception:
                    pass
            raise
        return self._finish(out, return_device, sync=True, hand_over=False)  # (a device result: the chunks die with this frame, after the sync)

    def _pinned_chunks(self, tensor, stream, per_step):
        """source of a plan's chunks out of one scene's stream in PAGE-LOCKED host memory, pre-drawn or (`stream`, a PinnedNoiseStream
        over `tensor`) still being drawn by infer_serial's scene-ahead feeder: every copy is queued at once on the copy stream and each
        segment of the loop is ordered after its chunk - the GPU starts after 5.7 MB instead of after the whole 734 MB, and no host core
        draws or copies anything while the loop runs."""
        flat = tensor.view(-1)

        def source(seg):
            lo, hi = seg.offset * per_step, (seg.offset + seg.draws) * per_step
            if stream is not None:
                stream.wait_until(hi)  # (only the first scene of a run ever waits here: the feeder works a whole scene ahead)
            return self.ctx.upload_pinned({"t": flat[lo:hi]}, hi - lo)

        return source

    def _run_numpy_stream(self, plan, per_step, chunk_steps, segment, out, return_device):
        """Reference contract: z comes from the GLOBAL NumPy RandomState, X_T first, then one draw per step (diffusion.py:303, 126).
        The stream is drawn chunk by chunk and each chunk is uploaded and enqueued at once, so the host RNG (edmp_amd.nprng: ~0.9 ms
        per step for 1024 rows on 16 cores; NumPy itself needs 3.3-4 ms) runs while the GPU denoises the previous chunk.  The numbers
        and their order are those of one big standard_normal call."""
        ctx = self.ctx
        # The draws go straight into PINNED host memory (a ring of staging buffers owned by the context), so the upload is
        # one asynchronous DMA on the copy stream - no pageable-memory staging copy on a host core, which the draw threads
        # need.  A staging buffer is reused only after the copy out of it has completed (event).  The draws run in ONE
        # background thread (the C helper releases the GIL), strictly in order, with two threads fewer than the CPU quota
        # (nprng.draw_threads): chunk i+1 is drawn while this thread uploads chunk i and enqueues its kernel launches.
        ring = ctx.pinned_ring(3, (int(chunk_steps) + 1) * per_step)
        nthr = nprng.draw_threads()
        trace = self.noise_trace = [] if os.environ.get("EDMP_NOISE_TRACE") else None  # per chunk: host timestamps (debug)
        t_call = time.perf_counter()

        def since():
            return time.perf_counter() - t_call

        def draw(i):
            slot = ring[i % len(ring)]
            t0 = since()
            if slot["event"] is not None:
                slot["event"].synchronize()  # the previous upload out of this buffer is done
            t1 = since()
            n = plan[i].draws * per_step
            nprng.standard_normal((n,), nthreads=nthr, out=slot["np"][:n])
            if trace is not None:
                trace.append(("draw", i, plan[i].t_hi - plan[i].t_lo, t0, t1, since()))
            return slot, n

        pool = ctx.draw_pool()  # ONE long-lived draw thread per context: its OpenMP team stays alive (and warm) between scenes
        i, pending, stamps = 0, pool.submit(draw, 0), ()

        def source(seg):
            nonlocal i, pending, stamps
            ta = since()
            slot, n = pending.result()
            tb = since()
            i += 1
            pending = pool.submit(draw, i) if i < len(plan) else None
            zd = ctx.upload_pinned(slot, n)  # copy stream; this context's stream waits for it
            stamps = (ta, tb, since())
            return zd

        def drain():
            if pending is not None:
                pending.result()

        def traced(zd, seg, X_out):
            segment(zd, seg, X_out)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(ctx.stream)
            trace.append(("main", i - 1, seg.t_hi - seg.t_lo, *stamps, since(), ev))

        return self._run_segments(plan, source, segment if trace is None else traced, out, return_device, drain)

    def _run(self, form, noise, streams, draws, pairs, guided, cn, ws, x0_rows, t_stop, zero_row0, chunk_steps, return_device):
        """The device-resident run behind denoise_guided and denoise_guided_scenes, on a bound model and guide (_prepare) and checked
        arguments.  `form`: what the two differ in (_Form).  `noise`: None - the global NumPy stream, drawn chunk by chunk beside the loop -
        or one stream of (draws, B, C, N) f64 per scene (a single-scene run: one), all pinned host tensors - `streams`: the
        PinnedNoiseStream still filling each, or None - or all host arrays / device tensors; not read when the form brings seeds.
        `pairs`: the start / goal arrays as the form's entry points take them.  Returns (rows, C, N) as _finish gives it."""
        ctx, T, t_stop = self.ctx, self.T, int(t_stop)
        rows, per = int(np.prod(form.lead)), (draws, form.lead[-1]) + cn
        per_step = rows * cn[0] * cn[1]
        rng = "" if form.seeds is None else "_rng"
        out = ctx.empty((rows,) + cn, torch.float64)
        sp, gp, zr = _capi.as_pd(pairs[0]), _capi.as_pd(pairs[1]), 1 if zero_row0 else 0
        if ws is not None:
            x0d = ctx.to_dev(ws.x0, torch.float64)

        def seed(*source):  # (eps,) or (seeds, renoise)
            name = f"edmp_sampler_seed{'_scenes' if form.kind == 'scenes' else ''}{rng}_dev"
            _capi.check(getattr(ctx.lib, name)(ctx.h, ptr(x0d), x0_rows, *source, *form.lead, sp, gp, guided, ws.t_start, None), name)

        def denoise(z, steps, X_out):  # steps: (t_stop,) - the whole run - or (t_hi, t_lo, init) - a segment
            name = f"edmp_denoise_{form.kind}{rng}{'_segment' if len(steps) > 1 else ''}_dev"
            _capi.check(getattr(ctx.lib, name)(ctx.h, z, *form.lead, sp, gp, guided, *steps, zr, ptr(X_out) if X_out is not None else None), name)

        def segment(zd, seg, X_out):
            init, z = 1 if seg.init else 0, ptr(zd)
            if ws is not None:  # the seed call is the run's init; every segment continues it
                eps, z = self._after_lead(zd, seg, ws, per_step)
                if init:
                    seed(eps)
                init = 0
            denoise(z, (seg.t_hi, seg.t_lo, init), X_out)

        def plan():
            return chunk_plan(T, t_stop, chunk_steps) if ws is None else warm_plan(ws.t_start, t_stop, ws.lead, chunk_steps)

        def gather(n, pieces):
            """the run's (n, rows, C, N) draws out of its streams' pieces: one scene's are its own, a scene batch's are placed scene by scene"""
            if form.place is None:
                return pieces[0]
            with torch.cuda.stream(ctx.stream):
                return form.place(ctx.empty((n, rows) + cn, torch.float64), [p.view((n,) + per[1:]) for p in pieces])

        def fits(k, x):
            if tuple(x.shape) != per or x.dtype != torch.float64:
                raise _noise_error("noise" if len(noise) == 1 else f"noise[{k}]", per, x)

        settled = form.settle or ws is not None  # a device result of a direct run is handed over after a host synchronisation
        if form.seeds is not None:  # the device source in every run form: no chunk plan, no pinned ring, no draw thread
            if ws is None:
                denoise(form.seeds, (t_stop,), out)
            else:  # a warm run: the seed call (eps = the stream's step-0 draw when re-noising) plus one segment
                try:
                    seed(form.seeds, 1 if ws.renoise else 0)
                    denoise(form.seeds, (ws.t_start, t_stop, 0), out)
                finally:
                    if form.settle:
                        ctx.sync()
            return self._finish(out, return_device, sync=settled)
        if noise is None:
            return self._run_numpy_stream(plan(), per_step, chunk_steps, segment, out, return_device)
        if _is_pinned_f64(noise[0]):  # uploaded in the same chunks as the on-the-fly stream, each scene's piece by DMA
            for k, x in enumerate(noise):
                fits(k, x)
            parts = [self._pinned_chunks(x, st, per_step // len(noise)) for x, st in zip(noise, streams)]
            return self._run_segments(plan(), lambda seg: gather(seg.draws, [part(seg) for part in parts]), segment, out, return_device)
        try:
            pieces = [ctx.adopt(x) if (isinstance(x, torch.Tensor) and x.is_cuda) else ctx.to_dev(x, torch.float64) for x in noise]
            for k, x in enumerate(pieces):
                fits(k, x)
            nd = gather(draws, pieces)
            if ws is None and draws == T + 1:
                denoise(ptr(nd), (t_stop,), out)
            else:  # resident streams that hold a part of the loop's draws - a warm run's, or X_T and the steps down to t_stop -: one segment
                segment(nd, Segment(T if ws is None else ws.t_start, t_stop, True, draws, 0), out)
        except BaseException:
            if form.settle:
                with contextlib.suppress(Exception):
                    ctx.sync()
            raise
        return self._finish(out, return_device, sync=settled)

    def denoise_guided(self, model, guide, traj_len, num_channels, guidance_schedule, batch_size=1, start=None, goal=None,
                       condition=True, benchmarking=False, *, noise=None, seed=0, t_stop=0, zero_row0=True, return_device=False,
                       chunk_steps=DEFAULT_CHUNK_STEPS, allreduce=None, warm_start=None):
        """diffusion.py:300-356.  ``noise``: optional pre-drawn (T+1,B,C,N) f64 ndarray / device tensor (default:
        drawn from the global NumPy RNG in the reference's order); ``noise="device"`` draws z on the GPU (Philox,
        ``seed``) — a non-parity mode without the host draw / upload; a ``DeviceNoise(seed)`` is that source for every run form,
        ``warm_start`` included (the string keeps its refusals).  ``allreduce``: this call is one row shard
        of a batch spread over several GPUs; an ``edmp_amd.dist.RcclAllReduce`` (native ncclAllReduce inside the device loop) or a
        callable that sums the f64 device scalar over ranks in place (edmp_amd.dist.allreduce_sum_; a Python callback per guided step).
        ``warm_start``: a WarmStart(x0, t_start, renoise) - the run covers steps t_start .. t_stop + 1 only, from x0 forward-noised to
        t_start (or from x0 itself); ``noise`` is then (lead + t_start - t_stop, B, C, N), the eps draw first when re-noising (lead = 1),
        from the same sources.
        Returns (B,C,N) f64 ndarray (a fresh copy)."""
        ws, cn = warm_start, (int(num_channels), int(traj_len))
        seeds = noise._for_run(None, allreduce) if isinstance(noise, DeviceNoise) else None
        draws, x0_rows = self.T + 1, None
        if ws is not None:
            x0_rows = self._check_warm(ws, t_stop, noise, allreduce, {cn: 1, (int(batch_size),) + cn: int(batch_size)})
            draws = ws.lead + ws.t_start - int(t_stop)
            if hasattr(noise, "shape") and tuple(noise.shape) != (draws, int(batch_size)) + cn:
                raise _noise_error("noise", (draws, int(batch_size)) + cn, noise)
        self._prepare(model, guide, batch_size, guidance_schedule, condition)
        pairs = _startgoal(start, goal, needed=bool(condition) or guide is not None)
        self._check_run(model, traj_len, num_channels, t_stop)
        if allreduce is not None and (noise is None or isinstance(noise, str)):
            raise ValueError("sharded runs take an explicit noise array (this rank's rows of the global stream)")
        stream = noise if isinstance(noise, PinnedNoiseStream) else None
        if stream is not None:
            noise = stream.tensor
        with self._sharded(allreduce) if allreduce is not None else contextlib.nullcontext():
            if isinstance(noise, str):
                if noise != "device":
                    raise ValueError("noise must be an array, a device tensor, None (NumPy stream) or 'device'")
                seeds = int(seed) & 0xFFFFFFFFFFFFFFFF
            form = _Form("guided", (batch_size,), seeds, None, settle=False)
            return self._run(form, None if noise is None else [noise], [stream], draws, pairs, 1 if guide is not None else 0, cn, ws, x0_rows, t_stop, zero_row0,
                             chunk_steps, return_device)

    def denoise_guided_scenes(self, model, batch, traj_len, num_channels, starts, goals, *, noise=None, t_stop=0, zero_row0=True, condition=True,
                              chunk_steps=DEFAULT_CHUNK_STEPS, return_device=False, guided=True, warm_start=None):
        """S scenes of B rows each planned in ONE device-resident loop (edmp_denoise_scenes_dev): what S calls of denoise_guided, one per
        scene of ``batch`` (a guide.SceneBatch), return - bit for bit - as an (S, B, C, N) f64 array.  ``starts`` / ``goals`` (S, 7).
        ``noise``: None = the S streams from the global NumPy RandomState in scene order (the state ends where S denoise_guided calls leave
        it); a list of S (T+1, B, C, N) arrays / device tensors; or a list of S pinned tensors / PinnedNoiseStreams, uploaded in chunks
        beside the loop.  ``zero_row0``: quirk Q3 on row 0 of every scene.  ``guided=False``: the unguided loop, per-scene conditioning.
        ``warm_start``: as in denoise_guided, x0 (S, C, N) - scene s's plan for all its rows - or (S, B, C, N); every scene's stream is then
        (lead + t_start - t_stop, B, C, N)."""
        from .guide import SceneBatch, _pairs

        if not isinstance(batch, SceneBatch):
            raise ValueError("batch must be a guide.SceneBatch")
        S, B, T = batch.n_scenes, batch.batch_size, self.T
        ws, cn = warm_start, (int(num_channels), int(traj_len))
        seeds = noise._for_run(S) if isinstance(noise, DeviceNoise) else None
        x0_rows = None
        if ws is not None:
            x0_rows = self._check_warm(ws, t_stop, noise, None, {(S,) + cn: S, (S, B) + cn: S * B})
        if model.ctx is not self.ctx or batch.ctx is not self.ctx:
            raise _capi.EdmpError("model, scene batch and diffuser must live on the same GPU")
        self._check_run(model, traj_len, num_channels, t_stop)
        if S * B > model.max_batch:
            raise ValueError(f"{S} scenes x {B} rows exceed the model's max_batch ({model.max_batch})")
        if starts is None or goals is None:
            if bool(condition) or bool(guided):
                raise ValueError("starts and goals are required when conditioning or guiding")
            starts = goals = np.zeros((S, 7))
        pairs = _pairs(S, starts, goals)
        if isinstance(noise, str):
            raise _capi.EdmpError("the device noise mode (noise='device') has no scene batch: pass NumPy-stream noise")
        per = (T + 1 if ws is None else ws.lead + ws.t_start - int(t_stop), B) + cn  # a warm run's streams hold exactly its draws, from every source
        streams = resident = None
        if seeds is None:
            if noise is not None and (not isinstance(noise, (list, tuple)) or len(noise) != S):
                raise ValueError(f"noise must be None or a list of {S} per-scene streams")
            if noise is None:
                # every scene's stream in scene order, as S serial calls draw them (each draws X_T and the steps down to t_stop + 1)
                if ws is None:
                    per = (T + 1 - int(t_stop),) + per[1:]
                noise = [nprng.standard_normal(per) for _ in range(S)]
            streams = [x if isinstance(x, PinnedNoiseStream) else None for x in noise]
            noise = [x.tensor if isinstance(x, PinnedNoiseStream) else x for x in noise]
            pinned = [_is_pinned_f64(x) for x in noise]
            if any(pinned) and not all(pinned):
                raise ValueError("noise: either every scene's stream is pinned host memory or none is")
            for k, x in enumerate(noise):
                if tuple(x.shape) != per:
                    raise _noise_error(f"noise[{k}]", per, x)
            resident = not all(pinned)
        self._prepare(model, batch if guided else None, None, None, condition)
        if resident and any(isinstance(x, torch.Tensor) and x.dtype != torch.float64 for x in noise):
            raise ValueError("noise: every scene's stream must be f64")
        form = _Form("scenes", (S, B), seeds, place_scene_rows, settle=True)
        return self._run(form, noise, streams, per[0], pairs, 1 if guided else 0, cn, ws, x0_rows, t_stop, zero_row0, chunk_steps, return_device).reshape((S, B) + cn)

    def denoise(self, model, traj_len, num_channels, start=None, goal=None, condition=True, *, batch_size=1, noise=None, warm_start=None):
        """diffusion.py:253-278 (unguided), batched; returns X[0] like the reference when batch_size == 1."""
        X = self.denoise_guided(model, None, traj_len, num_channels, None, batch_size=batch_size, start=start, goal=goal, condition=condition, noise=noise,
                                warm_start=warm_start)
        return X[0] if batch_size == 1 else X

    def denoise_step(self, model, guide, X, z, t, start, goal, guidance_schedule=None, zero_row0=True, allreduce=None):
        """One teacher-forced reverse step on host arrays: returns dict(eps, x_post, grad (mixed, or None), x_out).
        ``allreduce(tensor)``: optional in-place sum over ranks of the device scalar sum(g^2) (multi-GPU)."""
        ctx = self.ctx
        B, Cc, N = X.shape
        self._prepare(model, guide, B, guidance_schedule, condition=True)
        Xd = ctx.to_dev(np.array(X, dtype=np.float64), torch.float64)  # a fresh device tensor: updated in place below
        zd = ctx.to_dev(np.asarray(z, dtype=np.float64), torch.float64)
        s, g = _startgoal(start, goal, needed=True)
        eps = ctx.empty((B, Cc, N), torch.float32)
        xpost = ctx.empty((B, Cc, N), torch.float64)
        grad = ctx.empty((B, Cc, N - 2), torch.float64)
        _capi.check(ctx.lib.edmp_step_a_dev(ctx.h, ptr(Xd), ptr(zd), B, int(t), _capi.as_pd(s), _capi.as_pd(g), 1 if zero_row0 else 0, ptr(eps), ptr(xpost)), "edmp_step_a_dev")
        guided = guided_step(t)
        if guided and allreduce is not None:
            with torch.cuda.stream(ctx.stream):
                allreduce(self.sumsq_tensor())
        _capi.check(ctx.lib.edmp_step_b_dev(ctx.h, ptr(Xd), B, int(t), _capi.as_pd(s), _capi.as_pd(g), ptr(grad)), "edmp_step_b_dev")
        return dict(eps=ctx.to_host(eps), x_post=ctx.to_host(xpost), grad=ctx.to_host(grad) if guided else None, x_out=ctx.to_host(Xd))

    def device_noise(self, seed, step_index, batch_size, num_channels=7, traj_len=50) -> np.ndarray:
        """the (B,C,N) z tensor of ``noise="device"`` at step_index (0 = X_T, 1 + T - t = reverse step t)."""
        ctx = self.ctx
        out = ctx.empty((batch_size, num_channels, traj_len), torch.float64)
        _capi.check(ctx.lib.edmp_rng_normal_dev(ctx.h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step_index), batch_size, num_channels, traj_len, ptr(out)))
        return ctx.to_host(out)

    def sumsq_tensor(self) -> torch.Tensor:
        """zero-copy f64 view of the device scalar holding sum(g^2) of the last guided step."""
        p = self.ctx.lib.edmp_sumsq_ptr_dev(self.ctx.h)

        class _Holder:
            __cuda_array_interface__ = {"shape": (1,), "typestr": "<f8", "data": (int(p), False), "version": 2}

        return torch.as_tensor(_Holder(), device=self.ctx.device)
