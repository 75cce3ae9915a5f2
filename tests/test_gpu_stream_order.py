"""Stream ordering at every call that takes or returns GPU tensors (docs/LAB_NOTES.md §3), with the race made deterministic by
tests/stream_order.py: an input that is still poison when the call is made must have been adopted, a result cloned on the caller's stream at
once must have been handed over.  The relation checked is equality, bit for bit with NaN patterns, with the same call on host arrays (resp.
with the same call made without a hold); that the host-array result is right is what the other suites establish.

`caller` is torch's default stream or the side stream of the process (stream_order.side_stream: a stream the runtime runs beside the
contexts' own).  The side-stream variant is the deciding one; whether the default stream orders itself against the library's streams on its
own is a property of the runtime, and test_the_harness_sees_a_missing_wait records what it found for both ("harness" in the JSON) - the hold
is never lengthened to make the default-stream variant fail.  Measured on an MI355X (profiles/stream_order.json): torch's null stream does
NOT synchronise implicitly with the contexts' streams there - with either wait patched out both variants fail, each at every result.

A limit of the method: a call that synchronises with the host before it returns (success_rows, the loops' settled forms, IK) cannot be held
past that point from outside; its hand-over case holds by that synchronisation, and a torch op enqueued after it is covered by reading.

Every case certifies its own premise with an event recorded behind its hold: the hold was still running when the library first adopted a
late argument (resp. when the clones had been enqueued).  An attempt whose hold had ended - the host was paused past it - decides nothing
and is made again, three times at the most; the cases that never decided are listed under "undecided" in the JSON.  These are the hand-over
cases of the calls that synchronise before they return, and the one-at-a-time cases of SceneBatch's samplers behind the first argument.  An
undecided all-late case from the side stream fails.

With EDMP_STREAM_ORDER_OUT=<file> the measured call latencies, the hold derived from them, its calibrated unit count, per entry and caller
whether adoption and hand-over held, and the module's total time are written there as JSON (profiles/stream_order.json comes from such a run)."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import stream_order as S

pytestmark = pytest.mark.gpu
CALLERS = ("default", "side")
ADOPTED = [e.name for e in S.TABLE if e.device_args]
RETURNED = [e.name for e in S.TABLE if e.return_device]
IN_FLIGHT = [e.name for e in S.TABLE if e.in_flight]
RESULTS = {"adoption": {}, "hand_over": {}, "lane1": {}, "chain": {}, "harness": {}, "undecided": []}
_t0 = [None]


@pytest.fixture(scope="module", autouse=True)
def _record():
    _t0[0] = time.perf_counter()
    yield
    torch.cuda.synchronize()
    out = os.environ.get("EDMP_STREAM_ORDER_OUT")
    if out:
        cal = S.calibration()
        doc = {"what": "tests/test_gpu_stream_order.py: the hold of tests/stream_order.py and what held under it",
               "largest_latency_ms": cal["largest_latency_ms"], "hold_factor": cal["hold_factor"], "hold_floor_ms": S.HOLD_FLOOR_MS,
               "target_hold_ms": cal["target_hold_ms"], "measured_hold_ms": cal["measured_hold_ms"], "hold_units": cal["units"], "hold_kind": cal["kind"],
               "calibration_steps": cal["calibration_steps"], "side_stream_probes": cal.get("side_stream_probes"), "latency_ms": cal["latency_ms"], **RESULTS, "attempts_per_case_at_most": S.ATTEMPTS, "holds_enqueued": cal["holds"],
               "held_ms_enqueued": round(cal["holds"] * cal["measured_hold_ms"], 1), "module_seconds": round(time.perf_counter() - _t0[0], 2)}
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)


def decided(case, key, caller, must=True):
    """case() -> (..., decided): the first attempt whose premise held (stream_order.ATTEMPTS at the most; an attempt during which the
    host was paused past the hold decides nothing and is discarded - the outcome of a decided attempt does not depend on chance).  None
    decided: recorded under "undecided", and a failure where the case must decide - from the side stream.  From the default stream it need
    not: a call that makes the null stream wait for the device before it adopts anything sits out a hold placed there."""
    for _ in range(S.ATTEMPTS):
        out = case()
        if out[-1]:
            return out
    RESULTS["undecided"].append(key)
    assert not (must and caller == "side"), f"{key}: in {S.ATTEMPTS} attempts the hold had always ended before the call's work was enqueued: nothing was decided"
    return out


def check_adoption(entry, caller, which="base"):
    """all device arguments late at once, then - for an entry with several - one at a time with the others host arrays: a read placed in
    front of the adoption it relies on shows only there -> {late argument: result paths that differ}"""
    call = S.call_of(entry.name, which)
    assert set(call.slots) == set(entry.device_args), f"{entry.name}: the record states the device arguments {entry.device_args}, the call has {tuple(call.slots)}"
    bad = {}
    for slot in [None] + (list(call.slots) if len(call.slots) > 1 else []):
        # (one at a time a case need not decide: SceneBatch's samplers adopt their own state from the caller's stream and then copy host
        # arrays up, a blocking copy behind that wait - the hold is over before the later arguments are reached.  Recorded under "undecided".)
        bad[slot or "all"] = decided(lambda: S.adoption_differences(entry, caller, which, only=slot), f"adoption:{which}:{entry.name}[{caller}]:{slot or 'all'}", caller,
                                     must=slot is None)[0]
    return {k: v for k, v in bad.items() if v}


def check_hand_over(entry, caller, which="base"):
    """-> the result paths whose clone differs.  An entry that synchronises with the host before it returns sits out the hold and is never
    decided: it is recorded under "undecided" (its results are ordered by that synchronisation), not failed."""
    bad, device, held = decided(lambda: S.hand_over_differences(entry, caller, which), f"hand_over:{which}:{entry.name}[{caller}]", caller, must=False)
    assert device == sorted(entry.device_results), f"{entry.name}: the record states the device results {sorted(entry.device_results)}, the call returned {device}"
    return bad


@pytest.mark.parametrize("caller", CALLERS)
@pytest.mark.parametrize("name", ADOPTED)
def test_inputs_are_adopted(name, caller):
    bad = check_adoption(S.BY_NAME[name], caller)
    RESULTS["adoption"][f"{name}[{caller}]"] = not bad
    assert not bad, f"{name} called from the {caller} stream read a device argument before it was adopted; {{late argument: result paths that differ}} = {bad}"


@pytest.mark.parametrize("caller", CALLERS)
@pytest.mark.parametrize("name", RETURNED)
def test_results_are_handed_over(name, caller):
    bad = check_hand_over(S.BY_NAME[name], caller)
    RESULTS["hand_over"][f"{name}[{caller}]"] = not bad
    assert not bad, f"{name} called from the {caller} stream returned device tensors that the caller's stream is not ordered after (or read an input late): {bad}"


@pytest.mark.parametrize("caller", CALLERS)
def test_lane_contexts(caller):
    """the entries the driver runs in flight (scenes_in_flight), on lane 1 of the GPU: its own stream, model and guides"""
    bad = {}
    for name in IN_FLIGHT:
        e = S.BY_NAME[name]
        a, h = check_adoption(e, caller, "lane1"), check_hand_over(e, caller, "lane1")
        RESULTS["lane1"][f"{name}[{caller}]"] = dict(adoption=not a, hand_over=not h)
        if a or h:
            bad[name] = dict(adoption=a, hand_over=h)
    assert not bad, bad


# ---- the chain of the driver's finishing stages -------------------------------------------------------------------------------------------
def _clones(out):
    if isinstance(out, torch.Tensor):
        return out.clone()
    if isinstance(out, dict):
        return {k: (v.clone() if isinstance(v, torch.Tensor) and v.is_cuda else v) for k, v in out.items()}
    return out


def chain(r, owner, device):
    """denoise -> repair -> shortcut -> success -> select (fastest) -> time -> blend -> time_blended -> sample_blended of the chosen rows
    -> {stage: its result as the caller saw it at once}.  device=False: through host arrays.  device=True: every state stays on the device
    and the caller alternates between the default and the side stream from call to call (the new stream ordered after the old one, as a
    caller of torch owes it).  Per stage:
      our stream is held, the call is made, and its results are cloned on the caller's stream AT ONCE - these clones are what is compared:
        without the hand-over they are read before our kernel ran;
      then the caller's stream - the stream that produces what the next call receives - is held for TWO holds and the results are cloned
        again: these clones go into the next call.  They land one hold after the next stage's kernel would run if that stage did not adopt
        them (our stream carries one hold in front of it), so without the adoption it reads them unwritten.
    The noise of the first stage is late behind two holds for the same reason.
    This is a VALUE check: the device-resident chain gives the host chain's bits under that schedule.  What decides each stage's adoption
    and hand-over is its per-entry case above; no test shows the chain's own sensitivity (a wrong first stage would propagate to every
    later one anyway), and its first stage is called from torch's default stream, which side_stream() does not probe."""
    obj, ctx, scenes = r.obj(owner), r.ctx, owner == "scenes"
    streams, turn, stages = [S.caller_stream("default"), S.caller_stream("side")], [0], {}

    def step(name, f, *a, rd=True, **kw):
        if not device:
            stages[name] = f(*a, **kw)
            return stages[name]
        prev, cur = streams[turn[0] % 2], streams[(turn[0] + 1) % 2]
        turn[0] += 1
        cur.wait_stream(prev)
        S.hold(ctx.stream)
        with torch.cuda.stream(cur):
            out = f(*a, **kw, return_device=True) if rd else f(*a, **kw)  # (rd=False: a call that gives host values)
            stages[name] = _clones(out)
            if not rd:
                return out
            S.hold(cur)
            S.hold(cur)
            nxt = _clones(out)
            for v in (out.values() if isinstance(out, dict) else [out]):
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    v.record_stream(cur)  # (dropped below while the second clone is still pending on the caller's stream)
            return nxt

    if scenes:
        noise = list(r.scene_noise)
        if device:
            noise = S.late_all([S.ready(z, ctx.device) for z in noise], streams[0], holds=2)
        X = step("denoise", r.dif.denoise_guided_scenes, r.net, obj, 50, 7, r.starts, r.goals, noise=noise, t_stop=S.T_STOP)
        pair = (r.starts, r.goals)
    else:
        noise = S.late(r.noise, streams[0], holds=2) if device else r.noise
        X = step("denoise", r.dif.denoise_guided, r.net, obj, 50, 7, r.cfgs["guidance_schedule"], batch_size=4, start=r.start, goal=r.goal, noise=noise, t_stop=S.T_STOP)
        pair = (r.start, r.goal)
    X = step("repair", obj.repair_rows, X, *pair, iters=4)["trajectories"]
    X = step("shortcut", obj.shortcut_rows, X)["trajectories"]
    step("success", obj.success_rows, X)
    idx, _, _ = step("select", obj.select_rows if scenes else obj.select_row, *pair, X, prefer="fastest", rd=False)
    rows = [int(s * obj.batch_size + i) for s, i in enumerate(idx)] if scenes else [int(idx)]
    step("time", obj.time_rows, X)
    beta = step("blend", obj.blend_rows, X)["beta"]
    bprof = step("time_blended", obj.time_blended_rows, X, beta)
    step("sample_blended", obj.sample_blended_rows, X, bprof, 0.25, rows=rows)
    torch.cuda.synchronize()
    return stages


_host_chains = {}


def host_chain(owner):
    """the chain through host arrays: computed once, shared, left unchanged"""
    if owner not in _host_chains:
        _host_chains[owner] = chain(S.rig("base"), owner, False)
        assert np.isfinite(_host_chains[owner]["sample_blended"]["q"]).any(), "the chain's rows were not timed: the comparison would hold on NaN alone"
    return _host_chains[owner]


def device_chain_differences(owner):
    """the device-resident chain against the host chain -> the result paths ("stage.key") that differ.  Before it the free blocks of our
    stream's pool and of both callers' pools are poisoned at the sizes of the chain's results: a block recycled for an output or for a
    clone holds poison, not the host chain's (bit-identical) answer.  Flags that are bool on the host and int32 on the device compare by value."""
    r, host = S.rig("base"), host_chain(owner)
    S.calibration()
    sizes = sorted({v.nbytes for v in S.flatten(host).values() if isinstance(v, np.ndarray)})
    for stream in (None, S.caller_stream("default"), S.caller_stream("side")):
        S.poison_free_blocks(r.ctx, sizes, stream=stream)
    dev, want, bad = S.flatten(chain(r, owner, True)), S.flatten(host), []
    for k in sorted(set(dev) | set(want)):
        g, w = S.host_leaf(dev.get(k)), want.get(k)
        if isinstance(w, np.ndarray) and w.dtype == bool and isinstance(g, np.ndarray):
            g = g.astype(bool) if np.isin(g, (0, 1)).all() else g
        if k not in dev or k not in want or not S.same_bits(g, w):
            bad.append(k)
    return bad


@pytest.mark.parametrize("owner", ("guide", "scenes"))
def test_the_device_resident_chain(owner):
    bad = device_chain_differences(owner)
    RESULTS["chain"][owner] = not bad
    assert not bad, bad


# ---- the copy stream ----------------------------------------------------------------------------------------------------------------------
def test_copy_stream_paths():
    """upload_pinned and to_dev_overlapped behind a held copy stream: the kernel that reads the upload waits for it, and a pinned slot's
    event stays unsignalled while the hold lasts.  Only the upload_pinned half decides anything about the wait: to_dev_overlapped copies from
    pageable memory, a blocking copy, so the host sits out the hold and the data has landed before the kernel is enqueued - that half is a
    value check (the same bits behind a held copy stream), and it would pass without to_dev_overlapped's wait_stream."""
    from edmp_amd import _capi, franka
    from edmp_amd.runtime import ptr

    r = S.rig("base")
    ctx, X = r.ctx, r.X
    S.calibration()
    n, N = X.shape[0], X.shape[2]
    dh = np.ascontiguousarray(franka.dh_table_f64())

    def metrics(xd):
        out = ctx.empty((4, n), torch.float64)
        _capi.check(ctx.lib.edmp_metrics_rows_dev(ctx.h, ptr(xd), n, N, C.c_double(0.1), _capi.as_pd(dh), ptr(out)), "edmp_metrics_rows_dev")
        return out

    pinned = torch.empty(X.size, dtype=torch.float64, pin_memory=True)
    pinned.numpy()[:] = X.reshape(-1)

    def run(held):
        res, slot = {}, {"t": pinned, "event": None}
        for name, upload in (("to_dev_overlapped", lambda: ctx.to_dev_overlapped(X, torch.float64)), ("upload_pinned", lambda: ctx.upload_pinned(slot, X.size))):
            if held:
                with torch.cuda.stream(ctx.copy_stream):  # (the uploads allocate under the copy stream: poison what they will be handed)
                    torch.empty(X.size, dtype=torch.float64, device=ctx.device).fill_(float("nan"))
                ctx.copy_stream.synchronize()
                S.hold(ctx.copy_stream)
            xd = upload()
            out = metrics(xd)
            if held and name == "upload_pinned":
                res["event_signalled_under_the_hold"] = slot["event"].query()
            res[name] = ctx.to_host(out)
            del xd
        ctx.copy_stream.synchronize()
        res["event_signalled_after"] = slot["event"].query()
        return res

    ctx.to_dev_overlapped(X, torch.float64)  # (makes the copy stream)
    ctx.sync()
    assert ctx.copy_stream.cuda_stream not in (ctx.stream.cuda_stream, S.side_stream().cuda_stream)
    plain, held = run(False), run(True)
    assert np.isfinite(plain["to_dev_overlapped"]).all()
    for k in ("to_dev_overlapped", "upload_pinned"):
        assert S.same_bits(plain[k], held[k]) and S.same_bits(plain[k], plain["to_dev_overlapped"]), k
    assert held["event_signalled_under_the_hold"] is False and held["event_signalled_after"] is True and plain["event_signalled_after"] is True


# ---- the harness itself -------------------------------------------------------------------------------------------------------------------
def test_the_harness_sees_a_missing_wait(monkeypatch):
    """The comparisons above are not vacuous and the hold is long enough: with Context.adopt patched to return its argument without the
    wait, time_rows and batch_metrics compute on poison - their kernels have a defined non-finite path: no row is timed, every metric is
    NaN - and a profile whose duration alone is late gives sample_rows other samples; with Context.hand_over patched the same way the clones
    of time_rows' results are read before they were written.  These cases read allocated memory early, fault nothing, and each runs once
    (again only if the host was paused past the hold: the assertions are made on attempts whose premise held).  The side-stream variants
    decide; what the default stream does is recorded (torch's null stream may order itself against the library's streams on its own)."""
    from edmp_amd.runtime import Context

    seen = RESULTS["harness"]
    time_rows, metrics, sample_rows = (S.BY_NAME[n] for n in ("time_rows", "batch_metrics", "sample_rows"))
    with monkeypatch.context() as m:
        m.setattr(Context, "adopt", lambda self, t: t)
        for caller in CALLERS:
            for e in (time_rows, metrics):
                got, _ = decided(lambda: S.call_with_late_arguments(e, caller), f"missing_adopt:{e.name}[{caller}]", caller)
                seen[f"missing_adopt:{e.name}[{caller}]"] = S.differences(got, S.host_result(e.name))
                if caller == "side":  # the defined non-finite path: nothing is timed, every metric is NaN
                    assert all(np.isnan(got[k]).all() for k in (("duration",) if e is time_rows else got)) and (e is metrics or (got["limit"] == -1).all())
            key = f"missing_adopt:sample_rows:duration_alone[{caller}]"
            seen[key] = decided(lambda: S.adoption_differences(sample_rows, caller, only="profile.duration"), key, caller)[0]
    with monkeypatch.context() as m:
        m.setattr(Context, "hand_over", lambda self, t: t)
        for caller in CALLERS:
            key = f"missing_hand_over:time_rows[{caller}]"
            seen[key] = decided(lambda: S.hand_over_differences(time_rows, caller), key, caller)[0]
    torch.cuda.synchronize()
    print("[stream order] what the harness saw with the waits patched out:", json.dumps(seen))
    for key, bad in seen.items():
        if key.endswith("[side]"):
            assert bad, f"{key}: the wait was patched out and the comparison still held - the harness cannot see a missing wait"
    # and with the waits back in place the same cases hold
    for e in (time_rows, metrics):
        assert not check_adoption(e, "side")
    assert not check_hand_over(time_rows, "side")
