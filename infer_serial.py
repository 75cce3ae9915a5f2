#!/usr/bin/env python
"""infer_serial.py — the reference's driver surface (infer_serial.py:14-170) on the MI355X-native sampler.

    python infer_serial.py -c configs/cfg_c1_plumbing.yaml

Same flow: run config (YAML, schema of benchmark/cfgs/cfg1.yaml) -> guide plugins (guides/cfgs/guide<N>.yaml schema)
-> per-row guide_cfgs -> per scene: guide object, IK-goal filter (guide.cost at t=0, trust region 0.0008, nearest to
start), Diffusion.denoise_guided, choose_best_trajectory.  Differences forced by missing third-party assets, all
stated in DESIGN.md: scenes/IK goals are synthetic unless a dataset object is supplied, weights are random-init
unless <model_dir>/TemporalUNetModel<T>_N<traj_len>/weights_latest.pt exists, success is the geometric proxy
(pybullet absent)."""
import argparse
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch

from edmp_amd import dist as ED
from edmp_amd import evaluation as EV
from edmp_amd import franka
from edmp_amd import guide_cfg as GC
from edmp_amd.diffusion import DEFAULT_CHUNK_STEPS, DeviceNoise, Diffusion, PinnedNoiseStream, chunk_plan
from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch, pick_goal
from edmp_amd.runtime import get_context, lane_context
from edmp_amd.scenes import SyntheticDataset
from edmp_amd.temporalunet import TemporalUNet

CHECK_SUBSTEPS = 4  # the success check's configurations per segment (success_rows' default, which every call below takes)


def _ranks(device):
    """Launched under ``python -m torch.distributed.run --nproc-per-node N infer_serial.py ...`` (one process per GPU): join the
    process group and return (rank, world, this rank's device).  Backend "nccl" (= RCCL) when every local rank has its own GPU,
    EDMP_DIST_BACKEND=gloo lets the ranks share one (single-GPU test boxes), as in bench.py.  Outside a launcher: (0, 1, device)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1, device
    import torch.distributed as dist

    backend = os.environ.get("EDMP_DIST_BACKEND", "nccl")
    local, ngpu = int(os.environ.get("LOCAL_RANK", "0")), torch.cuda.device_count()
    if backend == "nccl" and ngpu < int(os.environ.get("LOCAL_WORLD_SIZE", world)):
        raise SystemExit(f"[infer_serial] {world} ranks over RCCL need one GPU each, this node shows {ngpu}: launch fewer ranks (or EDMP_DIST_BACKEND=gloo to share)")
    index = local if backend == "nccl" else local % max(ngpu, 1)
    torch.cuda.set_device(index)
    if not dist.is_initialized():
        dist.init_process_group(backend, **({"device_id": torch.device("cuda", index)} if backend == "nccl" else {}))
    return dist.get_rank(), dist.get_world_size(), f"cuda:{index}"


def scene_seed(seed, i):
    """the device noise seed of scene i of the cfg's order (i counts over all ranks) under ``--device-noise SEED``: a scene's stream is a
    function of (SEED, i) alone - not of the grouping, the lanes, the ranks or the scenes planned before it"""
    return (int(seed) + int(i) * 0x9E3779B97F4A7C15) % 2**64


class _NoiseFeeder:
    """Every scene's (T+1, B, C, N) noise stream, drawn IN SCENE ORDER from the global NumPy RandomState (so each
    scene sees the numbers the serial loop would give it) by ONE background thread into page-locked whole-scene buffers, ahead of the
    scene that consumes it; the planning threads upload their buffer by DMA.  Drawing on the calling thread instead serialised the
    loop on the host: 0.16 s of draws + a pageable 734 MB upload per 1024-row scene made two scenes in flight SLOWER than the serial
    loop (profiles/r05_problem_set.md).  Exactly `n_scenes` streams are drawn: the global state ends where the serial loop leaves it."""

    def __init__(self, ctx, n_scenes, shape, n_buffers):
        import queue
        import threading

        from edmp_amd import nprng

        n = int(np.prod(shape))
        cache = getattr(ctx, "_scene_noise_buffers", None)
        if cache is None or len(cache) < n_buffers or cache[0].numel() != n:
            cache = ctx._scene_noise_buffers = [torch.empty(n, dtype=torch.float64, pin_memory=True) for _ in range(n_buffers)]
        self.shape, self.free, self.ready = tuple(shape), queue.Queue(), queue.Queue()
        for b in cache[:n_buffers]:
            self.free.put(b)
        nthr = nprng.draw_threads()
        pieces = self.pieces(shape)

        def work():
            stream = None
            try:
                for _ in range(n_scenes):
                    b = self.free.get()
                    if b is None:
                        return
                    stream = PinnedNoiseStream(b.view(self.shape))
                    self.ready.put(stream)  # handed out at once: the consumer uploads each chunk as soon as it is drawn
                    flat, off = b.numpy(), 0
                    for m in pieces:  # piecewise draws continue the legacy stream exactly (the cached second gauss value travels in the state)
                        nprng.standard_normal((m,), nthreads=nthr, out=flat[off:off + m])
                        off += m
                        stream.publish(off)
            except BaseException as exc:  # surfaced by next() / by the consumer's wait
                if stream is not None:
                    stream.publish(stream.drawn, error=exc)
                self.ready.put(exc)

        self.thread = threading.Thread(target=work, name="edmp-scene-noise", daemon=True)
        self.thread.start()

    @staticmethod
    def pieces(shape):
        """doubles per published piece of one (T+1, B, C, N) stream: the chunks of the sampler's own plan, so that every watermark a consumer
        waits for is the end of a piece"""
        per_step = int(np.prod(shape[1:]))
        return [seg.draws * per_step for seg in chunk_plan(int(shape[0]) - 1, 0, DEFAULT_CHUNK_STEPS)]

    def next(self):
        """the next scene's stream (scene order): a PinnedNoiseStream over a pinned (T+1, B, C, N) f64 tensor, possibly still being drawn"""
        b = self.ready.get()
        if isinstance(b, BaseException):
            raise b
        return b

    def recycle(self, stream):
        self.free.put(stream.tensor.view(-1))

    def close(self):
        self.free.put(None)
        self.thread.join()


def repair_tally(rep, iters, margin):
    """what a repair_rows dict says about its rows, per row: moved (iterations > 0) and ended clear (the last evaluation had no active
    hinge term).  A row that stopped before `iters` stopped BECAUSE no hinge was active; one that used all of them is counted clear when
    its last clearance - over every tested configuration, start and goal included - is at least the margin as the kernel holds it (f32),
    which leaves out only a row whose pinned start or goal itself sits inside the margin."""
    it = np.asarray(rep["iterations"].cpu() if isinstance(rep["iterations"], torch.Tensor) else rep["iterations"])
    clr = np.asarray(rep["clearance"].cpu() if isinstance(rep["clearance"], torch.Tensor) else rep["clearance"])
    return it > 0, (it >= 0) & ((it < int(iters)) | (clr >= float(np.float32(margin))))


CERTIFY_KEYS = ("verdict", "segment", "fraction", "link", "bound")  # what the driver reads of certify_rows' dict


def certify_tally(cert, collision_free, idx, depth, margin):
    """what one scene's result says of the continuous certificate: the census of the rows' verdicts, the rows that the sampled success check
    passes and the certificate reports as hit, and the chosen plan's verdict with its bound (free) or its hit / first undecided interval"""
    v = np.asarray(cert["verdict"])
    out = dict(certify_depth=int(depth), certify_margin=float(margin), certify_rows={name: int(np.count_nonzero(v == k)) for k, name in enumerate(EV.CERTIFY_VERDICT_NAMES)},
               rows_passed_but_certified_hit=int(np.count_nonzero((v == 1) & np.asarray(collision_free, dtype=bool))), certify_verdict=EV.CERTIFY_VERDICT_NAMES[int(v[idx])])
    if v[idx] == 0:
        out.update(certify_bound=float(cert["bound"][idx]))
    elif v[idx] in (1, 2):
        out.update(certify_at=dict(segment=int(cert["segment"][idx]), fraction=float(cert["fraction"][idx]), link=franka.LINK_NAMES[int(cert["link"][idx])]))
    return out


def job_summary(results, world=1, self_collision=False, repair=False, shortcut=False, self_safe=False):
    """This rank's tallies; under a launcher the sum over all ranks (all_gather_object of five small integers per rank - the
    trajectories stay where they were planned).  Keys: scenes, success_proxy (the reference's tally), success_strict, rows_collision_free, rows."""
    mine = dict(scenes=len(results), success_proxy=sum(r["success_proxy"] for r in results), success_strict=sum(r["success_strict"] for r in results),
                rows_collision_free=sum(r["rows_collision_free"] for r in results), rows=sum(r["rows"] for r in results),
                planning_time_s=float(sum(r["planning_time_s"] for r in results)))
    if self_collision:  # (run(..., self_collision=True): every rank's results carry the keys)
        mine.update(self_collision_free=sum(r["self_collision_free"] for r in results), rows_self_collision_free=sum(r["rows_self_collision_free"] for r in results))
    if repair:  # (run(..., repair=ITERS): every rank's results carry the keys)
        mine.update(rows_repaired=sum(r["rows_repaired"] for r in results), rows_repair_clear=sum(r["rows_repair_clear"] for r in results))
    if shortcut:  # (run(..., shortcut=PASSES): every rank's results carry the key)
        mine.update(rows_shortcut=sum(r["rows_shortcut"] for r in results))
        if self_safe:  # (run(..., shortcut=PASSES, self_safe=True))
            mine.update(shortcut_self_rejected=sum(r["shortcut_self_rejected"] for r in results))
    if world <= 1:
        return dict(mine, ranks=1)
    import torch.distributed as dist

    parts = [None] * world
    dist.all_gather_object(parts, mine)
    out = {k: sum(p[k] for p in parts) for k in mine}
    out["ranks"] = world
    out["scenes_per_rank"] = [p["scenes"] for p in parts]
    return out


def _dataset(cfg):
    """the run config's own dataset.  The reference's types (datasets/load_test_dataset.py:15-38: 'global' | 'hybrid' | 'both' ->
    <path>/<type>_solvable_problems.pkl) are served from the JSON scripts/mpinets_pkl_to_json.py writes next to the pickle, when it is there"""
    d = cfg["dataset"]
    if d["dataset_type"] not in ("global", "hybrid", "both"):
        return SyntheticDataset(d["dataset_type"], d_path=d["path"], scene_types=d["scene_types"], num_scenes_per_type=d.get("num_scenes_per_type", 1))
    converted = os.path.join(d["path"], f"{d['dataset_type']}_solvable_problems.json")
    if not os.path.exists(converted):
        raise FileNotFoundError(f"{converted} not found: convert {d['dataset_type']}_solvable_problems.pkl with scripts/mpinets_pkl_to_json.py (IK goals via --ik-goals), "
                                "or use dataset_type: 'synthetic'")
    from edmp_amd.scenes import ProblemSetDataset

    return ProblemSetDataset(converted)


def _my_scenes(scene_types, dataset, max_scenes, rank, world):
    """this rank's scenes as (i, scene_type, scene_num), in the cfg's order (scene i of that order belongs to rank i mod world)"""
    mine, i = [], 0
    for scene_type in scene_types:
        for scene_num in range(dataset.data_nums[scene_type]):
            if max_scenes is not None and i >= max_scenes:
                break
            if i % world == rank:
                mine.append((i, scene_type, scene_num))
            i += 1
    return mine


def _lanes(job, base, k, model_dir, max_batch):
    """one (diffuser, denoiser) per scene in flight; the weights are replicated per context.  Lane 0 = the device's context `base`; further
    lanes are cached per (device, lane), not re-created per call"""
    model_name = model_dir + "TemporalUNetModel" + str(job.T) + "_N" + str(job.traj_len)
    if not os.path.exists(model_name):
        if job.verbose and job.rank == 0:
            print(f"[infer_serial] {model_name} not found: using a seeded random-init denoiser (no trained weights offline)")
        model_name = None
    return [(Diffusion(T=job.T, device=ctx), TemporalUNet(model_name=model_name, input_dim=job.num_channels, time_dim=32, dims=(32, 64, 128, 256, 512, 512), device=ctx, max_batch=max_batch))
            for ctx in (lane_context(base, j) for j in range(k))]


def _fetch(job, lane, scenes):
    """dataset.fetch_data per scene; with ik_seeds, the targets of the scenes that bring no goals are solved first, in one call"""
    ds = job.dataset
    if not job.iks:
        return [ds.fetch_data(scene_num=scene_num, scene_type=scene_type) for _, scene_type, scene_num in scenes]
    poses = [ds.target_pose(scene_num, scene_type) for _, scene_type, scene_num in scenes]
    need = [j for j, p in enumerate(poses) if p is not None]
    solved = dict(zip(need, job.iks[lane].solve_many([poses[j] for j in need])["goals"])) if need else {}
    return [ds.fetch_data(scene_num=scene_num, scene_type=scene_type, **({"goals": solved[j]} if j in solved else {})) for j, (_, scene_type, scene_num) in enumerate(scenes)]


def _goal_kw(job, scenes):
    """the goal term's constructor keywords, one dict per scene (empty without a goal-weighted guide: the guides are built as they
    were): the problems' own target poses in the frame ik_tool when every scene of the group carries one, else the pose of the picked goal"""
    if "sdf_goal_weight" not in job.guide_cfgs:
        return [{} for _ in scenes]
    probs = getattr(job.dataset, "problems", None)  # (ProblemSetDataset.target_pose answers None for a problem that brings its own IK goals)
    targets = [probs[scene_type][scene_num].get("target") if probs is not None and scene_type in probs else None for _, scene_type, scene_num in scenes]
    poses = [None if t is None else (t["xyz"], t["quaternion_wxyz"]) for t in targets]
    if all(p is not None for p in poses):
        return [dict(goal_target=(np.asarray(p[0], dtype=np.float64), np.asarray(p[1], dtype=np.float64)), goal_tool=job.ik_tool) for p in poses]
    return [dict(goal_tool=job.ik_tool) for _ in poses]


def _guide(job, ctx, data, goal_kw, bind=True):
    """the guide of one fetched scene on the context ctx.  obstacle_config = cuboids first, then cylinders as (r, r, h) boxes
    (datasets/load_test_dataset.py:141-149); the success check spawns the latter as true cylinders (infer_serial.py:159-163 ->
    lib/environment.py:249-268).  bind=False: host tables only, for a SceneBatch"""
    obstacle_config, _, _, num_cuboids, num_cylinders, _, _ = data
    kinds = np.concatenate([np.zeros(int(num_cuboids), dtype=np.int32), np.ones(int(num_cylinders), dtype=np.int32)])
    return IntersectionVolumeGuide(obstacle_config=obstacle_config, device=ctx, guide_cfgs=job.guide_cfgs, batch_size=job.total_batch_size, obstacle_kinds=kinds,
                                   mesh_dir=job.mesh_dir, bind=bind, **goal_kw)


def _meta(job, scene):
    """the head of a scene's result; `noise_seed` is the key device_noise adds to it (none without it)"""
    i, scene_type, scene_num = scene
    return dict(scene_type=scene_type, scene_num=scene_num, **({} if job.device_noise is None else {"noise_seed": scene_seed(job.device_noise, i)}))


class _Path:
    """What tells the serial loop from a scene group in the one scoring step (_score), the way guide._SlotObject's ``shape`` tells edmp_x
    from edmp_scenes_x: obj = the IntersectionVolumeGuide, shape (B,), the rows a host (B, C, N) array | obj = the SceneBatch, shape
    (S, B), the rows the (S, B, C, N) device state.  The serial loop asks the chosen-plan reports for the chosen row alone, a group for
    all rows in one call.  `stamps` collects the times that become the result's `timings`, in `timings()`'s order; _score leaves `picked_at`
    and `checked_at`, when the selection and the success check returned (where the serial loop's planning time and scene wall time end)."""

    def __init__(self, obj, shape):
        self.obj, self.shape, self.grouped, self.stamps = obj, shape, len(shape) == 2, {}
        self.select = obj.select_rows if self.grouped else obj.select_row

    def scenes(self, a):
        """a per-row (or per-scene) result of `obj` with the scene axis in front"""
        return a if self.grouped else np.asarray(a)[None]

    def chosen(self, X, idx):
        """-> (the rows the chosen-plan reports are asked for, per scene the chosen row's place in what they answer)"""
        return (X, idx) if self.grouped else (X[idx][None], [0])

    def interior(self, rows):
        """what sdf_rows / sdf_sweep_rows / sdf_self_rows take: a guide the interior waypoints, a batch the full state"""
        return rows if self.grouped else rows[:, :, 1:-1]

    def goal_rows(self, rows):
        """the goal report with the goal column handed over as well: the final tool pose's distance and angle"""
        return self.obj.sdf_goal_rows(rows, final=True) if self.grouped else self.obj.sdf_goal_rows(rows[:, :, 1:])

    def sweep_substeps(self, idx):
        """the substeps of the swept clearance: the rows' own where they carry the swept-clearance term (sample guide 104), else the success
        check's (success_rows' default) - for the chosen row of a guide; a batch takes its rows' own (None) as soon as one row carries the term"""
        if self.grouped:
            return None if self.obj.has_sweep_term else CHECK_SUBSTEPS
        d = self.obj._sdf
        return int(d["sweep_substeps"][idx]) if d["sweep_weight"][idx] > 0 else CHECK_SUBSTEPS

    def host(self, X):
        """the scored rows on the host, scene axis in front: a group's state comes back once, for the result dicts"""
        return self.obj.ctx.to_host(X) if self.grouped else X[None]

    def timings(self):
        order = (("noise_wait_s", "batch_metrics_s", "denoise_s", "repair_s", "shortcut_s", "certify_s", "denoise_s_is", "best_trajectory_s", "success_check_s") if self.grouped else
                 ("noise_wait_s", "denoise_s", "repair_s", "shortcut_s", "certify_s", "best_trajectory_s", "batch_metrics_s", "success_check_s"))
        return {k: self.stamps[k] for k in order if k in self.stamps}


def _score(job, on, X, starts, goals, tb):
    """THE scoring step of both loops, from the end of the denoising loop (at time tb) to what _result writes down: repair -> shortcut -> select_row(s)
    -> the metrics when the report wants them -> success_rows -> the chosen plans' sphere reports -> self_collision_rows, on the finished
    rows X of the path `on` (_Path).  Every call scores ALL rows of X - a group's (S, B, C, N) state stays on the device and is scored as
    one batch - but the chosen-plan reports, which the path says the rows of.  -> one record of scores per scene (the serial loop: one)."""
    obj, st, report = on.obj, on.stamps, job.ensemble_report
    moved = clear = None
    if job.repair:  # the whole batch / group in one launch, between the loop and the selection; everything behind it sees the repaired rows
        rep = obj.repair_rows(X, starts, goals, iters=job.repair, substeps=CHECK_SUBSTEPS, margin=job.repair_margin, step=job.repair_step, return_device=on.grouped)
        X = rep["trajectories"]
        moved, clear = (on.scenes(a) for a in repair_tally(rep, job.repair, job.repair_margin))
        st["repair_s"] = time.time() - tb
        tb = time.time()
    cut = cut_self = None
    if job.shortcut:  # likewise one launch, after the repair and before the selection; everything behind it sees the shortened rows
        safe = dict(self_pairs=True) if job.self_safe else {}  # (self_safe: a candidate must also keep the arm free of itself, under the guide's own pair mask)
        sh = obj.shortcut_rows(X, passes=job.shortcut, substeps=CHECK_SUBSTEPS, log_cap=0, return_device=on.grouped, **safe)
        X = sh["trajectories"]
        host = lambda v: np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)  # noqa: E731
        cut = on.scenes(host(sh["accepted"]) > 0)
        if job.self_safe:
            cut_self = on.scenes(host(sh["self_rejected"]))
        st["shortcut_s"] = time.time() - tb
        tb = time.time()
    cert = Xh = None
    if job.certify is not None:  # likewise one launch, on the rows the selection sees: the continuous certificate of every row (a report; nothing behind it reads it)
        Xh = on.host(X)  # (certify_rows is a host-only call: a group's state comes back here, once, and serves the result dicts below)
        out = obj.certify_rows(Xh if on.grouped else X, depth=job.certify, margin=job.certify_margin)
        cert = {k: on.scenes(out[k]) for k in CERTIFY_KEYS}
        st["certify_s"] = time.time() - tb
        tb = time.time()
    idx, vols, met = on.select(starts, goals, X, prefer=job.prefer)
    on.picked_at = tc = time.time()
    st["best_trajectory_s"] = tc - tb
    if report and met is None:  # (the metrics need no scene: one call over all rows)
        met = {k: v.reshape(on.shape) for k, v in EV.batch_metrics(X.reshape((-1,) + tuple(X.shape[-2:])), device=obj.ctx).items()}
        st["batch_metrics_s"] = time.time() - tc
    # success: pybullet execution (lib/environment.py:632-680) is unavailable -> exact link-box vs cuboid / cylinder
    # check along the interpolated trajectory, for EVERY row in one kernel (csrc/success.hip); the
    # scene's success is the chosen row's flag (infer_serial.py:165-168) under the reference's rule - no contact;
    # leaving the joint limits only prints there (lib/environment.py:659-661, 672) -, the stricter flag (also inside the
    # limits) and the batch rates are reported next to it, as is the guide's own (conservative, AABB) criterion
    td = time.time()
    chk = obj.success_rows(X)
    on.checked_at = te = time.time()
    st["success_check_s"] = te - td
    rows, place = on.chosen(X, idx)
    chosen = {}
    if report and obj.has_sdf_rows:  # (a run with an SDF guide: the sphere model's clearance, and the same at the success check's interpolants)
        chosen["min_clearance"] = obj.sdf_rows(on.interior(rows), starts, goals)["clearance"]
        chosen["min_swept_clearance"] = obj.sdf_sweep_rows(on.interior(rows), starts, goals, substeps=on.sweep_substeps(idx))["clearance"]
    if report and obj.has_self_term:
        chosen["min_self_clearance"] = obj.sdf_self_rows(on.interior(rows))["clearance"]
    goal = on.goal_rows(rows) if report and obj.has_goal_term else None
    selfcol = obj.self_collision_rows(X) if job.self_collision else None
    lead = lambda d: None if d is None else {k: on.scenes(v) for k, v in d.items()}  # noqa: E731
    of = lambda d, *at: None if d is None else {k: v[at] for k, v in d.items()}  # noqa: E731
    idx, vols, X, chk, met, selfcol, goal, chosen = on.scenes(idx), on.scenes(vols), (on.host(X) if Xh is None else Xh), lead(chk), lead(met), lead(selfcol), lead(goal), lead(chosen)
    timed = _time_plans(job, on, X, idx) if job.time_plan is not None else None
    return [SimpleNamespace(idx=int(i), vols=vols[s], trajectory=X[s][int(i)], met=of(met, s), selfcol=of(selfcol, s), chosen=of(chosen, s, place[s]), goal=of(goal, s, place[s]),
                            chk={k: (v if np.ndim(v) else int(v)) for k, v in of(chk, s).items()},  # (the per-row flags, and the scene's counts as ints)
                            repair=None if moved is None else (moved[s], clear[s]), shortcut=None if cut is None else cut[s], shortcut_self=None if cut_self is None else cut_self[s], timed=None if timed is None else timed[s],
                            certify=of(cert, s))
            for s, i in enumerate(idx)]


def _time_plans(job, on, X, idx):
    """the chosen plans - row idx[s] of the host state X (S, B, 7, N) - timed under the default joint velocity, acceleration and corner-jump
    limits (EV.time_rows_on, one launch for the group) -> per scene dict(duration_s, binding_constraints = how many waypoints each
    constraint binds), and with a period (job.time_plan a number) the sample count of the timed motion at that period, from the sampler
    itself (EV.sample_rows_on, one launch).  With job.blend (a deviation [rad]) the chosen plans' corners are blended under the exact
    collision check against their own scenes (blend_rows on the chosen rows alone, one launch) and the blended path is timed
    (EV.time_blended_rows_on): `blended_duration_s`, `corner_codes` (the census of the interior waypoints' blend codes), `blend_deviation_rad`
    and `blend_reach` are added, and a period samples the faster of the two motions (`sampled_motion`)."""
    obj, ctx = on.obj, on.obj.ctx
    plans = np.stack([X[s][int(i)] for s, i in enumerate(idx)])
    prof = EV.time_rows_on(ctx, plans)
    out = [dict(duration_s=float(d), binding_constraints={name: int(np.count_nonzero(lim == k)) for k, name in enumerate(EV.LIMIT_NAMES)})
           for d, lim in zip(prof["duration"], prof["limit"])]
    if job.blend is None:
        if job.time_plan is not True:
            count = EV.sample_rows_on(ctx, plans, prof, job.time_plan)["count"]
            for o, c in zip(out, count):
                o.update(time_period_s=float(job.time_plan), timed_samples=int(c))
        return out
    S, B, _, N = X.shape
    rows = [s * B + int(i) for s, i in enumerate(idx)]
    safe = dict(self_pairs=True) if job.self_safe else {}  # (self_safe: a try must also keep the arm free of itself, under the guide's own pair mask)
    bl = obj.blend_rows(X if on.grouped else X[0], deviation=job.blend, reach=job.blend_reach, substeps=CHECK_SUBSTEPS, rows=rows, **safe)
    beta, code = bl["beta"].reshape(S * B, N)[rows], bl["code"].reshape(S * B, N)[rows]
    bprof = EV.time_blended_rows_on(ctx, plans, beta)
    for o, d, c in zip(out, bprof["duration"], code):
        o.update(blended_duration_s=float(d), corner_codes={name: int(np.count_nonzero(c[1:-1] == k)) for k, name in enumerate(EV.BLEND_CODE_NAMES)},
                 blend_deviation_rad=float(job.blend), blend_reach=float(job.blend_reach))
    if job.self_safe:
        for o, h in zip(out, bl["self_hits"].reshape(S * B, N)[rows]):
            o.update(blend_self_rejected_tries=int(h.sum()))
    if job.time_plan is not True:
        faster = [s for s in range(S) if bprof["duration"][s] < prof["duration"][s]]  # (a NaN duration compares false: the polyline's count, 0)
        plain = [s for s in range(S) if s not in faster]
        for motion, listed, sample, p in (("blended", faster, EV.sample_blended_rows_on, bprof), ("polyline", plain, EV.sample_rows_on, prof)):
            if listed:
                for s, c in zip(listed, sample(ctx, plans, p, job.time_plan, rows=listed)["count"]):
                    out[s].update(time_period_s=float(job.time_plan), timed_samples=int(c), sampled_motion=motion)
    return out


def _result(job, meta, tm, sc, t0, plan_end, wall_end=None, scenes_in_launch=None):
    """THE result dict of one scene: meta and the timings tm, `scenes_in_launch` behind them for a group, the base keys from the scene's scores
    sc (_score), then what each extension adds, in this order.  plan_end: where the scene's "Planning Time" ends (infer_serial.py:108-157:
    guide construction + IK filter + sampling + best pick); wall_end=None: now.  A new report is added here and in _score / _Path, nowhere else."""
    idx, vols, chk, trajectory = sc.idx, sc.vols, sc.chk, sc.trajectory
    r = dict(**meta, timings=tm, **({} if scenes_in_launch is None else {"scenes_in_launch": scenes_in_launch}),
             best_row=idx, swept_volume=float(vols[idx]), success_proxy=int(chk["collision_free"][idx]), success_strict=int(chk["ok"][idx]),
             rows_collision_free=chk["rows_collision_free"], rows_ok=chk["rows_ok"], rows=chk["rows"], aabb_volume_zero=bool(ED.geometric_success(float(vols[idx]), trajectory)),
             first_collision_waypoint=int(chk["first"][idx]), path_length=EV.path_lengths(trajectory), sparc=EV.smoothness(trajectory), planning_time_s=plan_end - t0,
             scene_wall_s=(time.time() if wall_end is None else wall_end) - t0, trajectory=trajectory)
    r.update({k: float(v) for k, v in sc.chosen.items()})  # ensemble_report with an SDF guide: min_clearance, min_swept_clearance; with the self-clearance term: min_self_clearance
    if sc.goal is not None:  # the guide carries the goal term: the chosen plan's final tool pose against the target, in the reference evaluator's units (mpinets/metrics.py:364-385)
        r.update(position_error=100.0 * float(sc.goal["distance"]), orientation_error=float(np.degrees(sc.goal["angle"])))
    if sc.selfcol is not None:  # self_collision: self_collision_rows' dict of the scene's rows
        a, b = (int(v) for v in sc.selfcol["pair"][idx])
        r.update(self_collision_free=int(sc.selfcol["free"][idx]), rows_self_collision_free=int(np.count_nonzero(sc.selfcol["free"])),
                 first_self_collision_waypoint=int(sc.selfcol["first"][idx]), self_collision_pair=None if a < 0 else [franka.LINK_NAMES[a], franka.LINK_NAMES[b]])
    if sc.repair is not None:  # repair: (moved, clear) of the scene's rows (repair_tally)
        r.update(rows_repaired=int(sc.repair[0].sum()), rows_repair_clear=int(sc.repair[1].sum()), repair_iters=int(job.repair))
    if sc.shortcut is not None:  # shortcut: the scene's rows with at least one accepted span
        r.update(rows_shortcut=int(sc.shortcut.sum()), shortcut_passes=int(job.shortcut))
        if sc.shortcut_self is not None:  # self_safe: the candidates of the scene's rows that the self test alone rejected
            r.update(shortcut_self_rejected=int(sc.shortcut_self.sum()))
    if sc.timed is not None:  # time_plan: the chosen plan's timed motion
        r.update(sc.timed)
    if sc.certify is not None:  # certify: certify_rows' per-row arrays of the scene's rows
        r.update(certify_tally(sc.certify, chk["collision_free"], idx, job.certify, job.certify_margin))
    if job.prefer is not None:
        r["prefer"] = job.prefer
    if job.ensemble_report:
        r["ensemble"] = EV.ensemble_report(job.guide_numbers, job.guide_rows, vols, chk, sc.met)
    return r


def _plan(job, lane, guide, start_joints, goal_joints, noise, meta, tm, t0):
    """one prepared scene on its lane: the loop, the scoring step, the result"""
    diffuser, denoiser = job.lanes[lane]
    on = _Path(guide, (job.total_batch_size,))
    pinned = None
    if noise is not None and not isinstance(noise, DeviceNoise):  # this scene's stream, drawn ahead by the feeder into page-locked memory: uploaded in chunks beside the loop
        t_w = time.time()
        pinned = noise.result() if hasattr(noise, "result") else noise
        on.stamps["noise_wait_s"] = time.time() - t_w
        noise = pinned
    ta = time.time()
    trajectories = diffuser.denoise_guided(model=denoiser, guide=guide, batch_size=job.total_batch_size, traj_len=job.traj_len, num_channels=job.num_channels, condition=True,
                                           benchmarking=True, start=start_joints, goal=goal_joints, guidance_schedule=job.guide_cfgs["guidance_schedule"], noise=noise)
    tb = time.time()
    if pinned is not None:
        job.feeder.recycle(pinned)  # (denoise_guided returned host trajectories: the upload out of the buffer is long done)
    on.stamps["denoise_s"] = tb - ta
    sc, = _score(job, on, trajectories, start_joints, goal_joints, tb)
    return _result(job, meta, {**tm, **on.timings()}, sc, t0, on.picked_at, on.checked_at)


def _prepare_group(job, scenes):
    """guides + IK filter of a scene group (infer_serial.py:108-129, once per scene there): the guides are host tables only
    (bind=False), the SceneBatch is the one object on the device, and ONE filter_goals call picks every scene's goal.
    -> (batch, [(start, goal, meta, timings, t0) per scene]); guide_ctor_s / ik_filter_s are the GROUP's times"""
    data = _fetch(job, 0, scenes)
    t0 = time.time()
    batch = SceneBatch([_guide(job, job.lanes[0][0].ctx, d, gkw, bind=False) for d, gkw in zip(data, _goal_kw(job, scenes))])
    t1 = time.time()
    starts = np.stack([np.asarray(d[5], dtype=np.float64) for d in data])
    _, chosen, _ = batch.filter_goals(starts, [d[6] for d in data])
    t2 = time.time()
    what = f"group of {len(data)} scenes"
    return batch, [(d[5], goal_joints, _meta(job, scene), dict(guide_ctor_s=t1 - t0, guide_ctor_s_is=what, ik_filter_s=t2 - t1, ik_filter_s_is=what), t0)
                   for scene, d, goal_joints in zip(scenes, data, chosen)]


def _plan_group(job, batch, group):
    """k prepared scenes in one launch chain and one scoring step; per scene the serial loop's result keys.  denoise_s, repair_s,
    noise_wait_s, best_trajectory_s, batch_metrics_s and success_check_s are the whole group's calls"""
    diffuser, denoiser = job.lanes[0]
    on = _Path(batch, (len(group), job.total_batch_size))
    t_w = time.time()
    streams = [job.feeder.next() for _ in group] if job.feeder is not None else DeviceNoise(seeds=[g[2]["noise_seed"] for g in group])
    on.stamps["noise_wait_s"] = time.time() - t_w
    starts, goals = np.stack([g[0] for g in group]), np.stack([g[1] for g in group])
    ta = time.time()
    Xd = diffuser.denoise_guided_scenes(denoiser, batch, job.traj_len, job.num_channels, starts, goals, noise=streams, condition=True, return_device=True)
    tb = time.time()
    for st in streams if job.feeder is not None else ():
        job.feeder.recycle(st)  # (the call synchronised before it returned the device state: every upload out of the buffers is done)
    on.stamps.update(denoise_s=tb - ta, denoise_s_is=f"group of {len(group)} scenes")
    scores = _score(job, on, Xd, starts, goals, tb)
    return [_result(job, meta, {**tm, **on.timings()}, sc, t0, time.time(), scenes_in_launch=len(group)) for (_, _, meta, tm, t0), sc in zip(group, scores)]


def _serial_loop(job, mine, k):
    """the reference's loop, one scene after the other on k lanes: guide, IK-goal filter, then the lane plans the scene (k = 1: at once,
    the reference's order of events).  The feeder thread draws every scene's whole stream in scene order from the global RandomState, so
    every scene sees the numbers the reference's loop would give it (nothing else may draw from the global state while a run is in
    progress); pool.submit hands the scenes to the lanes in order, the feeder hands the streams out in the same order"""
    pending = []
    with ThreadPoolExecutor(max_workers=k) as pool:
        for scene in mine:
            lane = (scene[0] // job.world) % k
            while len(pending) >= k:  # the lane's previous scene (and every earlier one) is done before its context is reused
                _collect(job, pending.pop(0))
            data = _fetch(job, lane, [scene])[0]
            start_joints, all_ik_goals = data[5], data[6]
            t0 = time.time()
            guide = _guide(job, job.lanes[lane][0].ctx, data, _goal_kw(job, [scene])[0])
            t1 = time.time()
            # IK-goal filter                                                              infer_serial.py:117-129
            volumes = guide.cost(torch.tensor(all_ik_goals.reshape((-1, 7, 1))), 0, batch_size=all_ik_goals.shape[0]).sum(axis=(1, 2)).cpu().numpy()
            _, goal_joints = pick_goal(volumes, all_ik_goals, start_joints)
            t2 = time.time()
            meta = _meta(job, scene)
            noise = job.feeder.next() if job.feeder is not None else DeviceNoise(meta["noise_seed"])
            args = (job, lane, guide, start_joints, goal_joints, noise, meta, dict(guide_ctor_s=t1 - t0, ik_filter_s=t2 - t1), t0)
            if k == 1:
                _collect(job, _plan(*args))
            else:
                pending.append(pool.submit(_plan, *args))
        while pending:
            _collect(job, pending.pop(0))


def _print_scene(r, n, tally, prefix=""):
    """the lines of scene n's result r under the running tallies"""
    print(prefix + f"Scene {n} ({r['scene_type']}/{r['scene_num']}): planning {r['planning_time_s']:.2f} s, best row {r['best_row']}, swept volume "
          f"{r['swept_volume']:.4g}, geometric success (proxy, collision-free) {r['success_proxy']} ({r['rows_collision_free']}/{r['rows']} rows of the batch); "
          f"also within the joint limits {r['success_strict']} ({r['rows_ok']}/{r['rows']})   running {tally.success}/{n} (strict {tally.strict}/{n})")
    for line in EV.format_ensemble_report(r.get("ensemble", ())):
        print(line)
    if "min_clearance" in r:  # (a run with an SDF guide: the sphere model's smallest clearance along the chosen plan)
        print(f"    chosen plan: minimum sphere clearance {r['min_clearance']:.4f} m")
    if "min_swept_clearance" in r:  # (the same at the configurations the success check interpolates between the waypoints)
        print(f"    chosen plan: minimum swept sphere clearance {r['min_swept_clearance']:.4f} m")
    if "min_self_clearance" in r:  # (the guide carries the self-clearance term: the sphere model's smallest distance to itself)
        print(f"    chosen plan: minimum self clearance {r['min_self_clearance']:.4f} m")
    if "position_error" in r:  # (the guide carries the goal term: the final tool pose against the target)
        print(f"    chosen plan: position_error {r['position_error']:.3f} cm, orientation_error {r['orientation_error']:.3f} deg")
    if "rows_repaired" in r:
        print(f"    repair ({r['repair_iters']} iterations at most): {r['rows_repaired']}/{r['rows']} rows moved, {r['rows_repair_clear']}/{r['rows']} ended clear")
    if "rows_shortcut" in r:
        print(f"    shortcut ({r['shortcut_passes']} passes at most): {r['rows_shortcut']}/{r['rows']} rows shortened"
              + (f"; {r['shortcut_self_rejected']} candidates rejected by the self-collision test alone" if "shortcut_self_rejected" in r else ""))
    if "certify_rows" in r:
        c = r["certify_rows"]
        at = r.get("certify_at")
        print(f"    certificate (depth {r['certify_depth']}, margin {r['certify_margin']:g} m): rows free {c['free']}, hit {c['hit']}, undecided {c['undecided']}, invalid "
              f"{c['invalid']}; {r['rows_passed_but_certified_hit']} rows pass the sampled check and are certified hit; chosen plan: {r['certify_verdict']}"
              + (f", every link box farther than {r['certify_bound']:.4g} m from every obstacle" if "certify_bound" in r else "")
              + (f" at segment {at['segment']}, fraction {at['fraction']:g}, {at['link']}" if at else ""))
    if "duration_s" in r:
        census = ", ".join(f"{k} {v}" for k, v in r["binding_constraints"].items() if v)
        print(f"    chosen plan: duration_s {r['duration_s']:.3f} under the joint velocity / acceleration / corner limits; waypoints bound by: {census}"
              + (f"; {r['timed_samples']} samples at {r['time_period_s']:g} s" if "timed_samples" in r else ""))
        if "blended_duration_s" in r:
            census = ", ".join(f"{k} {v}" for k, v in r["corner_codes"].items() if v)
            print(f"    chosen plan: blended_duration_s {r['blended_duration_s']:.3f} with corner blends within {r['blend_deviation_rad']:g} rad of the polyline "
                  f"(reach {r['blend_reach']:g}) under the exact collision check; corners: {census}"
                  + (f"; the samples are the {r['sampled_motion']} motion's" if "sampled_motion" in r else "")
                  + (f"; {r['blend_self_rejected_tries']} corner tries rejected by the self-collision test alone" if "blend_self_rejected_tries" in r else ""))
    if "self_collision_free" in r:
        print(f"    self-collision free {r['self_collision_free']} ({r['rows_self_collision_free']}/{r['rows']} rows of the batch)   running {tally.self_free}/{n}")
        if "ensemble" in r:
            print("    chosen plan: " + ("no self-collision" if r["self_collision_pair"] is None else
                                         f"self-collision of {r['self_collision_pair'][0]} and {r['self_collision_pair'][1]} at waypoint {r['first_self_collision_waypoint']}"))


def _collect(job, fut):
    """a finished scene (or the future of one): stamped, kept, tallied, printed"""
    r = fut.result() if hasattr(fut, "result") else fut
    r["done_at"] = time.time()
    job.results.append(r)
    job.tally.success += r["success_proxy"]  # the reference's tally: collision-free (infer_serial.py:165-168 on lib/environment.py:672)
    job.tally.strict += r["success_strict"]
    job.tally.self_free += r.get("self_collision_free", 0)
    if job.verbose:
        _print_scene(r, len(job.results), job.tally, "" if job.world == 1 else f"[rank {job.rank}] ")


def _print_summary(summary):
    print(f"[infer_serial] {summary['scenes']} scenes on {summary['ranks']} rank(s): success (proxy, collision-free) {summary['success_proxy']}/{summary['scenes']}, "
          f"strict {summary['success_strict']}/{summary['scenes']}, rows collision-free {summary['rows_collision_free']}/{summary['rows']}")
    if "self_collision_free" in summary:
        print(f"[infer_serial] self-collision free {summary['self_collision_free']}/{summary['scenes']}, rows {summary['rows_self_collision_free']}/{summary['rows']}")
    if "rows_repaired" in summary:
        print(f"[infer_serial] repair: {summary['rows_repaired']}/{summary['rows']} rows moved, {summary['rows_repair_clear']}/{summary['rows']} ended clear")
    if "rows_shortcut" in summary:
        print(f"[infer_serial] shortcut: {summary['rows_shortcut']}/{summary['rows']} rows shortened"
              + (f", {summary['shortcut_self_rejected']} candidates rejected by the self-collision test alone" if "shortcut_self_rejected" in summary else ""))


def run(cfg_path, dataset=None, max_scenes=None, verbose=True, scenes_in_flight=1, shard_scenes=True, scenes_per_launch=1, ensemble_report=False, prefer=None,
        ik_seeds=0, ik_tool=None, ik_seed=0, self_collision=False, device_noise=None, repair=0, repair_margin=0.02, repair_step=0.02, shortcut=0,
        time_plan=None, blend=None, blend_reach=0.4, self_safe=False, certify=None, certify_margin=0.0):
    """The reference's scene loop (infer_serial.py:95-170).  Under ``torch.distributed.run`` (one process per GPU, extension: the
    reference is one process) the scenes are dealt round-robin to the ranks - scene i of the cfg's order goes to rank i mod world -
    and nothing is exchanged until `job_summary` adds the tallies up: scenes are independent problems, this is the problem set's natural
    shard (SURVEY.md 8e "replicas + final gather").  Every rank draws from its OWN process-global NumPy RandomState, as N separate
    runs of the reference would (the reference never seeds it, infer_serial.py has no np.random.seed).  ``scenes_in_flight`` > 1 (an extension; the reference is serial) plans
    that many scenes concurrently on one GPU, each on its own context / stream / host thread: every launch of the sampler is one
    wave of 256 workgroups, a second independent scene fills its dispatch gaps and kernel tails (+7-9 % throughput measured,
    bench.py: two_scenes_in_flight).  Per-scene results are identical to the serial loop's: scenes are prepared in order on the
    calling thread and each scene's noise is drawn - by ONE background feeder thread, a whole scene ahead, serial loop included - from the
    global NumPy RandomState in scene order.  While a run is in progress nothing else may draw from (or seed) the global RandomState: the
    feeder reads and advances it from its own thread (np.random.get_state / set_state are not atomic).

    ``scenes_per_launch`` = k > 1 (an extension) plans k consecutive scenes of this rank in ONE device-resident loop
    (Diffusion.denoise_guided_scenes over a guide.SceneBatch): the group's guides are built as host tables only, the batch is the one
    object bound on the device and picks every scene's goal in one call (SceneBatch.filter_goals; the candidate volumes are summed in
    f64 there, so a goal can differ from the serial loop's only where a volume lies within f32 summation rounding of the trust-region
    threshold), the group is planned in one call, then the finished state stays on the device and every scene's best row and success are picked from its own rows by the
    batch's own scoring calls (SceneBatch.select_rows / success_rows: one launch per step for the group; a config that lists an SDF guide
    plans its SDF rows inside the batch, and with ensemble_report one SceneBatch.sdf_rows call gives every scene's `min_clearance`).  Per-scene results equal the serial loop's bit
    for bit; the last group may be smaller.  The model is built for k * rows, and the feeder keeps 2k whole-scene pinned buffers
    (k = 2 at 1024 rows: 4 x 734 MB page-locked).  Each result carries `scenes_in_launch`; its `denoise_s` is the GROUP's time.
    Not combined with scenes_in_flight > 1.

    ``ensemble_report`` (an extension) scores EVERY row of each scene's batch on the GPU (evaluation.batch_metrics: the path lengths and
    SPARC of lib/metrics.py, which the reference's driver never calls) and adds `ensemble` to the scene's result: one entry per guide of
    the cfg with its rows' collision-free / ok counts, best row, minimum swept volume and the mean / median metrics of its collision-free
    rows (evaluation.ensemble_report).  ``prefer`` = "shortest" | "smoothest" (an extension) picks the plan with
    IntersectionVolumeGuide.select_row - among the rows within the trust region of the minimum swept volume, the shortest joint path /
    the smoothest - instead of the first arg-min, and records `prefer` in the result.  Without either the results are the reference-shaped ones.

    ``ik_seeds`` = n > 0 (an extension; 0 = off, nothing changes) plans a problem set whose problems carry a target pose and no IK goals:
    the candidates come from edmp_amd.ik.FrankaIK (batched numerical IK on the GPU, n seeds per target from a private RandomState(ik_seed),
    never the global stream the feeder is advancing); with scenes_per_launch the group's targets are solved in one solve_many call.
    ``ik_tool`` is the frame the targets are given in, behind the joint-7 frame (ik.tool_frame: None = the reference's end-effector chain,
    "flange", "hand" or a (4, 4) array - MPiNets' right_gripper offset is the caller's to pass).  Problems that carry goals keep them.

    ``self_collision`` (an extension; off: every result and every printed line is what it was) checks EVERY row of each batch for
    self-collision on the GPU (IntersectionVolumeGuide / SceneBatch.self_collision_rows: the link boxes against each other under
    franka.self_collision_pairs(); a scene group in one call) and adds to the scene's result `self_collision_free` (the chosen plan's
    flag, tallied like success), `rows_self_collision_free`, `first_self_collision_waypoint` and `self_collision_pair` (the chosen plan's
    first colliding pair as two franka.LINK_NAMES, None when free); with ensemble_report the chosen plan's flag and pair are printed.

    ``device_noise`` = SEED (an extension; None: the NumPy stream, as above) draws every scene's noise on the GPU (diffusion.DeviceNoise:
    Philox inside the step tail, explicitly no parity with the reference's stream): scene i of the cfg's order - i counts over all ranks -
    runs under ``scene_seed(SEED, i)``, recorded as `noise_seed` in its result, so its plan is the same whatever scenes_per_launch,
    scenes_in_flight, the number of ranks and the scenes planned before it.  No feeder thread is started, no page-locked scene buffer is
    allocated and the global RandomState is neither read nor advanced.

    A run config with a goal-weighted SDF guide (``hyperparameters.sdf.goal_weight``, sample guide 103) hands every guide its target: the
    problem's own target pose (``dataset.target_pose``, given in the frame ``ik_tool``) when it carries one, else the pose of the picked
    goal configuration; with ensemble_report the chosen plan's ``position_error`` [cm] and ``orientation_error`` [deg] of the final tool
    pose against it are added and printed, the units of the reference's evaluator (mpinets/metrics.py:364-385).

    With ensemble_report a run with an SDF guide also adds ``min_swept_clearance`` next to ``min_clearance``: the chosen plan's smallest
    sphere clearance over the joint-space interpolants the success check tests between the waypoints (sdf_sweep_rows; the row's own
    ``sweep_substeps`` where it carries the swept-clearance term, sample guide 104, else the check's CHECK_SUBSTEPS).

    ``repair`` = ITERS > 0 (an extension; 0 = off: nothing is launched and every printed and returned value is what it was) sends the whole
    finished batch through repair_rows after the loop and before the selection and the success check (IntersectionVolumeGuide.repair_rows;
    a scene group through SceneBatch.repair_rows in one launch): at most ITERS projected descent steps of ``repair_step`` on the sphere
    model's hinge at ``repair_margin`` over the waypoints and the CHECK_SUBSTEPS - 1 interpolants per segment that the success check tests.
    Everything behind it sees the repaired rows.  Each result adds `rows_repaired` (rows that moved), `rows_repair_clear` (rows whose last
    evaluation had no active hinge, repair_tally) and `repair_iters`; the per-scene line and the summary print the two counts.

    ``time_plan`` (an extension; None = off: nothing is launched and every printed and returned value is what it was): True times each scene's
    chosen plan under Franka's joint velocity and acceleration limits and an illustrative corner velocity-jump limit (evaluation.time_rows:
    the fastest rest-to-rest motion along the plan's own polyline) and adds `duration_s` and `binding_constraints` (waypoints bound by each
    constraint) to the result; a number is also the period [s] at which that motion is sampled (evaluation.sample_rows), adding
    `time_period_s` and `timed_samples`.  ``prefer`` = "fastest" picks, inside the trust region, the row with the shortest such duration.

    ``blend`` = DEVIATION [rad] (an extension; None = off: nothing is launched and every printed and returned value is what it was; needs
    ``time_plan``) also blends the chosen plan's corners (IntersectionVolumeGuide / SceneBatch.blend_rows on the chosen rows: parabolic
    blends within DEVIATION of the polyline per joint and at most ``blend_reach`` <= 0.45 of a segment long, each accepted only if the
    success check's own test clears its CHECK_SUBSTEPS + 1 configurations) and times the blended path (evaluation.time_blended_rows),
    adding `blended_duration_s`, `corner_codes` (how many interior waypoints got each blend code), `blend_deviation_rad` and `blend_reach`
    next to `duration_s`; with a period the faster of the two motions is the one sampled and `sampled_motion` names it.  The selection
    does not see blended durations.

    ``shortcut`` = PASSES > 0 (an extension; 0 = off: nothing is launched and every printed and returned value is what it was) sends the
    whole batch through shortcut_rows after the repair and before the selection (IntersectionVolumeGuide.shortcut_rows; a scene group
    through SceneBatch.shortcut_rows in one launch): at most PASSES passes of joint-space shortcuts, each accepted only if the success
    check's own test passes at the configurations the check will test on it (CHECK_SUBSTEPS), so a row that is collision-free stays so.
    Self-collision is not part of that test unless ``self_safe`` is set: ``self_collision`` tallies after the stage.  Everything behind it
    sees the shortened rows.
    Each result adds `rows_shortcut` (rows with an accepted span) and `shortcut_passes`, and `shortcut_s` to the timings; the per-scene
    line and the summary print the count.

    ``self_safe`` (an extension; False = off: nothing new is launched, printed or returned; needs ``shortcut`` or ``blend``) passes
    self_pairs=True to those two stages: a shortcut candidate or a corner blend must also keep every masked pair of the arm's link boxes
    apart at the configurations it is tested at (the guide's own pair mask, the one ``self_collision`` checks under), so a row that is
    self-collision free before the stages is self-collision free after them.  Adds `shortcut_self_rejected` (the candidates of the
    scene's rows that the obstacle test passed and the self test rejected) with ``shortcut`` and `blend_self_rejected_tries` (the same
    for the chosen plan's corner tries) with ``blend``.

    ``certify`` = DEPTH in 0..10 (an extension; None = off: nothing is launched, printed or returned) sends the whole batch through
    certify_rows after the repair and the shortcuts and before the selection (a scene group through SceneBatch.certify_rows in one launch):
    the continuous collision certificate of every row over its whole joint-space polyline, with ``certify_margin`` [m] of clearance asked.
    It is a report - the selection and the success check do not read it.  Each result adds `certify_rows` (the census of free / hit /
    undecided / invalid rows), `rows_passed_but_certified_hit` (rows that success_rows passes and the certificate reports as hit),
    `certify_verdict` of the chosen plan with its `certify_bound` (free) or `certify_at` (segment, fraction, link of the hit or of the first
    undecided interval), `certify_depth`, `certify_margin`, and `certify_s` to the timings."""
    t_enter = time.time()
    kl = int(scenes_per_launch)
    if kl < 1:
        raise ValueError(f"scenes_per_launch must be >= 1, got {scenes_per_launch}")
    if kl > 1 and int(scenes_in_flight) > 1:
        raise ValueError("scenes_per_launch > 1 and scenes_in_flight > 1 do not combine: choose one")
    repair = int(repair)
    if repair < 0:
        raise ValueError(f"repair must be >= 0 iterations (0 = off), got {repair}")
    if time_plan is not None and time_plan is not True:
        time_plan = float(time_plan)
        if not (np.isfinite(time_plan) and time_plan > 0):
            raise ValueError(f"time_plan must be None (off), True, or a sample period > 0 [s], got {time_plan}")
    if blend is not None:
        blend, blend_reach = float(blend), float(blend_reach)
        if time_plan is None:
            raise ValueError("blend needs time_plan: the blended motion is reported next to the timed one")
        if not (np.isfinite(blend) and blend > 0):
            raise ValueError(f"blend must be None (off) or a deviation > 0 [rad], got {blend}")
        if not 0 < blend_reach <= 0.45:
            raise ValueError(f"blend_reach must lie in (0, 0.45], got {blend_reach}")
    if certify is not None:
        certify, certify_margin = int(certify), float(certify_margin)
        if not 0 <= certify <= 10:
            raise ValueError(f"certify must be None (off) or a depth in 0..10, got {certify}")
        if not (np.isfinite(certify_margin) and certify_margin >= 0):
            raise ValueError(f"certify_margin must be finite and >= 0 [m], got {certify_margin}")
    shortcut = int(shortcut)
    if shortcut < 0:
        raise ValueError(f"shortcut must be >= 0 passes (0 = off), got {shortcut}")
    self_safe = bool(self_safe)
    if self_safe and not shortcut and blend is None:
        raise ValueError("self_safe needs shortcut or blend: it is the self-collision test of those two stages")
    if device_noise is not None:
        DeviceNoise(device_noise)  # (an integer in [0, 2^64), or it raises)
    cfg = GC.load_yaml(cfg_path)
    model = cfg["model"]
    rank, world, device = _ranks(model["device"]) if shard_scenes else (0, 1, model["device"])
    if dataset is None:
        dataset = _dataset(cfg)
    guide_cfgs = GC.guide_cfgs_from_run_cfg(cfg, base_dir=os.path.dirname(os.path.abspath(cfg_path)) + "/..")
    if prefer not in (None, "shortest", "smoothest", "fastest"):
        raise ValueError(f"prefer must be None, 'shortest', 'smoothest' or 'fastest', got {prefer!r}")
    guide_numbers = [int(n) for n in cfg["guide"]["guides"]]
    job = SimpleNamespace(  # what the functions above share: the config's constants, the options, the dataset, the lanes and the running tallies
        T=model["T"], traj_len=model["traj_len"], num_channels=model["num_channels"], mesh_dir=model.get("mesh_dir"), guide_cfgs=guide_cfgs,
        total_batch_size=guide_cfgs["total_batch_size"], guide_numbers=guide_numbers,
        guide_rows=GC.split_rows(int(cfg["guide"]["total_rows"]), len(guide_numbers)) if cfg["guide"].get("total_rows") else guide_cfgs["batch_size_per_guide"],
        dataset=dataset, rank=rank, world=world, verbose=verbose, prefer=prefer, ensemble_report=ensemble_report, self_collision=self_collision, device_noise=device_noise,
        repair=repair, repair_margin=repair_margin, repair_step=repair_step, shortcut=shortcut, certify=certify, certify_margin=certify_margin, time_plan=time_plan, blend=blend, blend_reach=blend_reach, self_safe=self_safe, ik_tool=ik_tool, iks=[], feeder=None, results=[], tally=SimpleNamespace(success=0, strict=0, self_free=0))
    k = max(1, int(scenes_in_flight))
    base = get_context(device)
    job.lanes = _lanes(job, base, k, model["model_dir"], max_batch=job.total_batch_size * kl)
    ik_seeds = int(ik_seeds)
    if ik_seeds < 0:
        raise ValueError(f"ik_seeds must be >= 0, got {ik_seeds}")
    if ik_seeds > 0 and hasattr(dataset, "target_pose"):
        from edmp_amd.ik import FrankaIK

        job.iks = [FrankaIK(lane[0].ctx, n_seeds=ik_seeds, seed=ik_seed, tool=ik_tool) for lane in job.lanes]  # one solver per lane (a lane's context is only touched while its previous scene is done)
    mine = _my_scenes(cfg["dataset"]["scene_types"], dataset, max_scenes, rank, world)
    # the noise of EVERY scene comes from the feeder thread, one whole scene ahead (round 6: the serial loop too - drawing chunk by chunk
    # beside the GPU had no margin left once a reverse step took 0.92 ms: a slower host capped the scene loop, BENCH_r05 0.947 x value)
    # (the device source needs none of it: no thread, no page-locked buffer, no draw from the global state)
    if mine and device_noise is None:
        job.feeder = _NoiseFeeder(base, len(mine), (job.T + 1, job.total_batch_size, job.num_channels, job.traj_len), 2 * kl if kl > 1 else k + 1)
    run.last_setup_s = time.time() - t_enter  # config, dataset, model load / upload: per run, not per scene
    try:
        if kl > 1:
            for g0 in range(0, len(mine), kl):
                for r in _plan_group(job, *_prepare_group(job, mine[g0:g0 + kl])):
                    _collect(job, r)
        else:
            _serial_loop(job, mine, k)
    finally:
        if job.feeder is not None:
            job.feeder.close()
    if world > 1 or verbose:
        run.last_summary = job_summary(job.results, world, self_collision, bool(repair), bool(shortcut), self_safe)
        if verbose and rank == 0:
            _print_summary(run.last_summary)
    return job.results


def main(argv=None):
    parser = argparse.ArgumentParser(prog="Benchmarking Diffusion", description="Benchmarking with IK on Test sets")
    parser.add_argument("-c", "--cfg_path", type=str, default="./configs/cfg_c1_plumbing.yaml")
    parser.add_argument("--scenes-in-flight", type=int, default=1, help="plan this many scenes concurrently on the GPU (extension; the reference is serial)")
    parser.add_argument("--scenes-per-launch", type=int, default=1, help="plan this many consecutive scenes in one device-resident loop (extension; "
                                                                             "the model is built for that many times the rows)")
    parser.add_argument("--max-scenes", type=int, default=None, help="stop after this many scenes of the cfg's order (all ranks together)")
    parser.add_argument("--seed", type=int, default=None, help="np.random.seed(seed + rank) before the loop (the reference never seeds; for repeatable runs)")
    parser.add_argument("--device-noise", type=int, default=None, metavar="SEED", help="draw the noise on the GPU (Philox, no parity with the NumPy stream): scene i of the "
                                                                                        "cfg's order runs under scene_seed(SEED, i), whatever the grouping, the lanes and the ranks (extension)")
    parser.add_argument("--results-json", type=str, default=None, help="write this rank's per-scene results (without the trajectories) and the job summary "
                                                                       "to PATH (rank 0) / PATH.rank<r> (other ranks)")
    parser.add_argument("--ensemble-report", action="store_true", help="score every row of each batch on the GPU (path lengths, SPARC) and report, per guide of the "
                                                                       "ensemble, its collision-free rows and their metrics (extension; adds `ensemble` to the results)")
    parser.add_argument("--prefer", choices=("shortest", "smoothest", "fastest"), default=None, help="among the rows within the trust region of the minimum swept volume pick the "
                                                                                             "shortest joint path / the smoothest plan / the plan with the shortest timed motion "
                                                                                             "instead of the first arg-min (extension)")
    parser.add_argument("--ik-seeds", type=int, default=0, help="solve the IK of problems that carry a target pose and no goals on the GPU, from this many "
                                                                  "seeds per target (extension; 0 = off: such a problem set raises as before)")
    parser.add_argument("--ik-tool", type=str, default=None, help="the frame the targets are given in: 'flange', 'hand', or a JSON / .npy file holding a (4, 4) "
                                                                    "frame behind the joint-7 frame (default: the reference's end-effector chain)")
    parser.add_argument("--self-collision", action="store_true", help="check every row of each batch for self-collision on the GPU (link boxes against each other) "
                                                                      "and tally the chosen plans' flags (extension; adds `self_collision_free` to the results)")
    parser.add_argument("--repair", type=int, default=0, metavar="ITERS", help="after the loop and before the selection, repair every row of each batch by at most "
                                                                                "ITERS projected descent steps on the swept sphere-clearance cost (extension; 0 = off)")
    parser.add_argument("--repair-margin", type=float, default=0.02, help="the clearance [m] that the repair asks of every tested configuration")
    parser.add_argument("--repair-step", type=float, default=0.02, help="the repair's step size (a joint moves by at most 0.02 rad per iteration)")
    parser.add_argument("--time-plan", type=float, nargs="?", const=True, default=None, metavar="PERIOD", help="time the chosen plan under the joint velocity, acceleration "
                        "and corner velocity-jump limits (the fastest rest-to-rest motion along its polyline) and report its duration_s and which constraint binds "
                        "how many waypoints; with PERIOD [s] also the sample count of that motion at the period (extension; off: nothing changes)")
    parser.add_argument("--shortcut", type=int, default=0, metavar="PASSES", help="after the repair and before the selection, shorten every row of each batch by at most "
                                                                                    "PASSES passes of joint-space shortcuts, each accepted only under the exact collision check "
                                                                                    "(extension; 0 = off)")
    parser.add_argument("--blend", type=float, default=None, metavar="DEVIATION", help="with --time-plan: blend the chosen plan's corners by parabolic blends that stay "
                        "within DEVIATION [rad] of the polyline per joint and pass the exact collision check, and report blended_duration_s and the census of "
                        "the corner codes next to duration_s; with a PERIOD the faster of the two motions is sampled (extension; off: nothing changes)")
    parser.add_argument("--self-safe", action="store_true", help="with --shortcut and / or --blend: a shortcut candidate or a corner blend must also keep the arm's "
                        "link boxes apart (the pair mask of --self-collision), so a row that is self-collision free before those stages is after them; "
                        "reports the candidates and corner tries that this test alone rejected")
    parser.add_argument("--certify", type=int, nargs="?", const=6, default=None, metavar="DEPTH", help="after the repair and the shortcuts and before the selection, certify every "
                        "row of each batch collision-free over its WHOLE joint-space polyline (conservative advancement, at most DEPTH halvings per segment, "
                        "default 6): per scene the census of free / hit / undecided / invalid rows, the rows that the sampled success check passes and the "
                        "certificate reports as hit, and the chosen plan's verdict (extension; off: nothing is launched or printed)")
    parser.add_argument("--certify-margin", type=float, default=0.0, metavar="M", help="the clearance [m] that a certified row keeps from every obstacle")
    parser.add_argument("--blend-reach", type=float, default=0.4, metavar="R", help="the largest part of a neighbouring segment that a blend may take, in (0, 0.45]")
    args = parser.parse_args(argv)
    if args.blend is not None and args.time_plan is None:
        parser.error("--blend requires --time-plan")
    if args.self_safe and not args.shortcut and args.blend is None:
        parser.error("--self-safe requires --shortcut or --blend")
    ik_tool = args.ik_tool
    if ik_tool is not None and ik_tool not in ("flange", "hand"):
        if ik_tool.endswith(".npy"):
            ik_tool = np.load(ik_tool)
        else:
            with open(ik_tool) as f:
                ik_tool = np.asarray(json.load(f), dtype=np.float64)
    rank = int(os.environ.get("RANK", "0"))
    if args.seed is not None:
        np.random.seed(args.seed + rank)
    results = run(args.cfg_path, scenes_in_flight=args.scenes_in_flight, max_scenes=args.max_scenes, scenes_per_launch=args.scenes_per_launch,
                  ensemble_report=args.ensemble_report, prefer=args.prefer, ik_seeds=args.ik_seeds, ik_tool=ik_tool, self_collision=args.self_collision,
                  device_noise=args.device_noise, repair=args.repair, repair_margin=args.repair_margin, repair_step=args.repair_step, shortcut=args.shortcut, time_plan=args.time_plan,
                  certify=args.certify, certify_margin=args.certify_margin, blend=args.blend, blend_reach=args.blend_reach, self_safe=args.self_safe)
    if args.results_json:
        rows = [{k: v for k, v in r.items() if k != "trajectory"} for r in results]
        with open(args.results_json + ("" if rank == 0 else f".rank{rank}"), "w") as f:
            json.dump({"rank": rank, "summary": getattr(run, "last_summary", None), "scenes": rows}, f, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    return results


if __name__ == "__main__":
    main()
