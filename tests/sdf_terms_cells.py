"""The cells of tests/golden/sdf_terms_parent.json, defined once: what the host path of the SDF guide's optional terms (guide_cfg,
guide.sdf_tables, guide.scene_batch_tables, dist.shard_guide_cfgs) and the library behind it give for a fixed set of inputs.
scripts/record_sdf_terms_parent.py evaluates them with the PARENT commit's package, tests/test_sdf_terms_host.py and
tests/test_gpu_sdf_terms.py with this checkout's, and hold the two equal.  Nothing here names a module that only one of the two has:
the seven keys are spelled out, and edmp_amd is whatever package sys.path finds first."""
import hashlib
import json
import os

import numpy as np

from tests import sdf_reference as R

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdf_terms_parent.json")
T, BPG = R.T, 4
#            guide_cfgs key, host-table key
TERM_KEYS = (("sdf_self_weight", "self_weight"), ("sdf_self_margin", "self_margin"), ("sdf_goal_weight", "goal_weight"), ("sdf_goal_rotation", "goal_rotation"),
             ("sdf_goal_window", "goal_window"), ("sdf_sweep_weight", "sweep_weight"), ("sdf_sweep_substeps", "sweep_substeps"))
GUIDE_SETS = {"101": [101], "102": [102], "103": [103], "104": [104], "1_103_104": [1, 103, 104], "all_terms": ["all"], "no_sdf": [1, 11]}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest(d):
    """a dict of arrays / scalars -> its key list in order and, per key, [dtype, shape, sha256 of the bytes]"""
    return {"keys": list(d), "items": {k: [str(np.asarray(v).dtype), list(np.shape(v)), sha(np.asarray(v))] for k, v in d.items()}}


def guide_dict(n):
    """a built-in guide, or "all": guide 103 (self + goal) with the sweep term on top - all three terms on one guide"""
    from edmp_amd import guide_cfg as GC

    if n != "all":
        return GC.load_guide_dict(n)
    d = GC.catalog_guide_dict(103)
    d["index"] = 105
    d["hyperparameters"]["sdf"].update(sweep_weight=0.5, sweep_substeps=3)
    return d


def cfgs_of(guides, bpg=BPG):
    from edmp_amd import guide_cfg as GC

    return GC.build_guide_cfgs([guide_dict(n) for n in guides], bpg, T)


def half_extents():
    from edmp_amd import franka

    return franka.link_half_extents(franka.PLACEHOLDER_LINK_EXTENTS)


def scene_dict(cfgs, tables, seed):
    """one scene of scene_batch_tables as SceneBatch.__init__ puts it together, from host tables alone"""
    from edmp_amd import guide as G

    rc, cc, ce = G.row_classes(np.asarray(cfgs["clearance"], dtype=np.float64), np.asarray(cfgs["expansion"], dtype=np.float64))
    sc = dict(obstacle_config=R.make_case(seed, 1, 1, 3, 1)["obstacle_config"], row_class=rc, clearance=cc, expansion=ce,
              method=np.asarray(cfgs["guidance_method"], dtype=np.float32).reshape(-1), grad_norm=np.asarray(cfgs["grad_norm"], dtype=np.float64).reshape(-1),
              guidance_schedule=np.ascontiguousarray(np.asarray(cfgs["guidance_schedule"], dtype=np.float64)))
    if "sdf_rows" in cfgs:
        sc.update(sdf_rows=tables["rows"], sdf_margin=tables["margin"], smoothness=tables["smooth"], **{c: tables[h] for c, h in TERM_KEYS})
    return sc


def host_cells():
    from edmp_amd import guide as G
    from edmp_amd.dist import shard_guide_cfgs, shard_rows

    out = {}
    for name, guides in GUIDE_SETS.items():
        cfgs = cfgs_of(guides)
        B = cfgs["total_batch_size"]
        tb = G.sdf_tables(cfgs, B, T, half_extents())
        out[name] = {"cfgs": digest(cfgs), "tables_default": digest(tb), "tables_custom": digest(G.sdf_tables(cfgs, B, T, half_extents(), spheres=R.custom_spheres())),
                     "batch": digest(G.scene_batch_tables([scene_dict(cfgs, tb, 3), scene_dict(cfgs, tb, 4)])),
                     "shards": [digest(shard_guide_cfgs(cfgs, *shard_rows(B, r, 2))) for r in range(2)]}
    return out


def verdict(fn):
    """"accepted" with the digest of what came back, or the exception's type"""
    try:
        d = fn()
    except Exception as e:  # noqa: BLE001 - the type is the record
        return type(e).__name__
    return "accepted " + hashlib.sha256(json.dumps(digest(d), sort_keys=True).encode()).hexdigest()[:16]


SCALARS = (-1.0, float("nan"), float("inf"), -float("inf"), True, False, "1", None, 0, 1, 2, 2.5, 3.0, 64, 65, -3, 1j, [1.0, 2.0], np.float64(0.5), np.float32(2.0),
           np.int64(3), np.int32(0), np.array(3), np.array(0.25), np.array([1.0]), np.bool_(True))
PAIRS = ([0.1, -0.1], [0.1], [float("nan"), 0.0], [0.0, float("inf")], "ab", (0.1, 0.2, 0.3), np.array([0.01, 0.02]), [True, False], 0.5, None, [[0.1, 0.2]], (1, 2),
         ["0.1", "0.2"])
HYPER = {"self": ("self_weight", "self_margin"), "goal": ("goal_weight", "goal_rotation", "goal_window"), "sweep": ("sweep_weight", "sweep_substeps")}


def cfg_probes():
    """name -> callable: build_guide_cfgs of guides [1, X, 2] where X carries one odd value - under the term's weight > 0 (guide "all"),
    under weight 0 and without a weight (guide 101) - and a weight > 0 on a guide that is not an 'sdf' guide"""
    from edmp_amd import guide_cfg as GC

    def run(base, edit, where=1):
        def fn():
            d = [GC.catalog_guide_dict(1), guide_dict(base), GC.catalog_guide_dict(2)]
            d[where]["hyperparameters"].setdefault("sdf", {}).update(edit)
            return GC.build_guide_cfgs(d, 3, T)
        return fn

    out = {}
    for term, keys in HYPER.items():
        for key in keys:
            for i, v in enumerate(PAIRS if key == "self_margin" else SCALARS):
                tag = f"{key}[{i}]={v!r}"
                out[f"weighted {tag}"] = run("all", {key: v})
                if key != keys[0]:
                    out[f"weight 0 {tag}"] = run("all", {keys[0]: 0.0, key: v})
                    out[f"no weight {tag}"] = run(101, {key: v})
        for v in (1.0, True, 0.0, np.float64(2.0)):
            out[f"{keys[0]}={v!r} on an iv guide"] = run(101, {keys[0]: v}, where=2)
    return out


def table_probes():
    """name -> callable: sdf_tables of the row arrays of guides [1, "all", 101] x 2 rows with one array edited.  Rows 0-1 are no SDF
    rows, rows 2-3 carry every weight, rows 4-5 are SDF rows without one"""
    from edmp_amd import guide as G

    good = cfgs_of([1, "all", 101], 2)
    half = half_extents()

    def run(key, make):
        def fn():
            c = dict(good)
            c[key] = make(np.array(good[key], copy=True))
            return G.sdf_tables(c, 6, T, half)
        return fn

    def put(row, v, dtype=None):
        def make(a):
            a = a if dtype is None else a.astype(dtype)
            a[row] = v
            return a
        return make

    out = {}
    for key, _ in TERM_KEYS:
        for row in (0, 2, 4):  # no SDF row / weighted row / SDF row under weight 0
            for v in (-0.5, float("nan"), float("inf"), 0, 1, 2, 2.5, 64, 65, -3):
                out[f"{key}[{row}]={v!r} as float64"] = run(key, put(row, v, np.float64))
                if v == v and abs(v) != float("inf") and v == int(v):
                    out[f"{key}[{row}]={v!r} as int64"] = run(key, put(row, v, np.int64))
        out[f"{key} wrong shape"] = run(key, lambda a: np.zeros(3))
        out[f"{key} transposed rank"] = run(key, lambda a: a[None])
        out[f"{key} as bool"] = run(key, lambda a: a.astype(bool))
        out[f"{key} as str"] = run(key, lambda a: a.astype(str))
        out[f"{key} as object"] = run(key, lambda a: a.astype(object))
        out[f"{key} as list"] = run(key, lambda a: a.tolist())
        out[f"{key} as float32"] = run(key, lambda a: a.astype(np.float32))
        out[f"{key} as complex"] = run(key, lambda a: a.astype(np.complex128))
        out[f"{key} absent"] = lambda key=key: G.sdf_tables({k: v for k, v in good.items() if k != key}, 6, T, half)
    return out


def host_record():
    return {"cells": host_cells(), "cfg_probes": {k: verdict(f) for k, f in cfg_probes().items()}, "table_probes": {k: verdict(f) for k, f in table_probes().items()}}


# ---- GPU cells --------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
GPU_SEEDS = (0, 1)  # make_case seeds of the two scenes; find_gpu_seeds() searched them, gpu_case asserts that assert_margins accepts them
L, N_OBSTACLES, N_CYLINDERS = 6, 3, 1
GPU_GUIDES = ["all", 11]  # the 'sdf' guide with all three terms (goal_window 8 > L: the ramp's clamp; sweep_substeps 3) and an 'sv' guide that normalises
T_CHECK = R.T_CHECK
STEPS = 6  # guided steps of the scene-batch run (three of them guided: diffusion.guided_step)


def gpu_case(k=0, seed=None):
    """scene k: joints (8, 7, L), start, goal, three obstacles (the last a cylinder), the 8-row cfgs; the obstacle part sits away from
    its decision boundaries at t = 0 and at T_CHECK on the SDF rows"""
    cfgs = cfgs_of(GPU_GUIDES)
    B = cfgs["total_batch_size"]
    inp = R.make_case(GPU_SEEDS[k] if seed is None else seed, B, L, N_OBSTACLES, N_CYLINDERS)
    sph = R.case_spheres("default")
    rows = np.flatnonzero(cfgs["sdf_rows"])
    for t, margin in ((0, np.zeros(B)), (T_CHECK, cfgs["sdf_margin"][:, T_CHECK - 1])):
        ev = R.evaluate(inp["joints"][rows], inp["start"], inp["goal"], inp["obstacle_config"], inp["kinds"], sph, margin[rows], cfgs["smoothness"][rows], want_grad=False)
        R.assert_margins(ev, f"scene {k} t={t}")
    return dict(inp, cfgs=cfgs, B=B)


def find_gpu_seeds():
    return tuple(R.find_seed(lambda s, k=k: gpu_case(k, s), first) for k, first in ((0, 0), (1, GPU_SEEDS[0] + 1)))


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def build_guide(case, **kw):
    from edmp_amd import franka
    from edmp_amd.guide import IntersectionVolumeGuide

    return IntersectionVolumeGuide(case["obstacle_config"], DEV, case["cfgs"], case["B"], link_mesh_extents=franka.PLACEHOLDER_LINK_EXTENTS, obstacle_kinds=case["kinds"], **kw)


def reports(obj, X, starts, goals, t):
    """the four report dicts of a guide (X = interior waypoints) or a batch (X = the full state), every value as float.hex"""
    out = {"sdf_rows": obj.sdf_rows(X, starts, goals, t), "sdf_self_rows": obj.sdf_self_rows(X, t), "sdf_goal_rows": obj.sdf_goal_rows(X, t),
           "sdf_sweep_rows": obj.sdf_sweep_rows(X, starts, goals, t)}
    return {name: {k: hexes(v) for k, v in d.items()} for name, d in out.items()}


def gpu_guide_cells():
    from tests.sdf_gpu import gradient_and_sumsq

    case = gpu_case(0)
    guide = build_guide(case)
    out = {}
    for t in (0, T_CHECK):
        G, sq = gradient_and_sumsq(guide, case["joints"], case["start"], case["goal"], t)
        assert np.array_equal(G, guide.get_gradient(case["joints"], case["start"], case["goal"], t))
        out[f"t={t}"] = {"gradient_sha256": sha(G), "sumsq": float(sq).hex(), "reports": reports(guide, case["joints"], case["start"], case["goal"], t)}
    return out


def gpu_batch_cells():
    import torch  # noqa: F401

    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import SceneBatch
    from edmp_amd.temporalunet import TemporalUNet
    from tests.util import TINY_DIMS

    cases = [gpu_case(0), gpu_case(1)]
    B, N = cases[0]["B"], 50
    net = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=W.init_state_dict(5, 7, 32, TINY_DIMS), max_batch=64)
    batch = SceneBatch([build_guide(c, bind=False) for c in cases])
    starts, goals = np.stack([c["start"] for c in cases]), np.stack([c["goal"] for c in cases])
    rs = np.random.RandomState(77)
    noise = [rs.standard_normal((T + 1, B, 7, N)) for _ in cases]
    X = Diffusion(T, DEV).denoise_guided_scenes(net, batch, N, 7, starts, goals, noise=noise, t_stop=T - STEPS)
    return {"state_sha256": sha(X), **{f"t={t}": reports(batch, X, starts, goals, t) for t in (0, T_CHECK)}}


def gpu_refusals():
    """(rc, edmp_last_error()) of the argument refusals that the three terms' refusal tests provoke on the setters and the reports: every
    one returns before anything is launched"""
    import ctypes as C

    import torch

    from edmp_amd import _capi
    from edmp_amd.guide import SceneBatch
    from edmp_amd.runtime import ptr

    case = gpu_case(0)
    cfgs, B = case["cfgs"], case["B"]
    plain_cfgs = {k: v for k, v in cfgs_of([1, 11]).items()}
    plain = build_guide(dict(case, cfgs=plain_cfgs))
    plain._bind()
    ctx = plain.ctx
    lib, h = ctx.lib, ctx.h
    pd, pi = (lambda a: _capi.as_pd(np.ascontiguousarray(a, dtype=np.float64))), (lambda a: _capi.as_pi32(np.ascontiguousarray(a, dtype=np.int32)))
    mask = np.ascontiguousarray(plain._self_pairs)
    sw, sm = cfgs["sdf_self_weight"], cfgs["sdf_self_margin"]
    gw, gr, gk = cfgs["sdf_goal_weight"], cfgs["sdf_goal_rotation"], cfgs["sdf_goal_window"]
    ww, wk = cfgs["sdf_sweep_weight"], cfgs["sdf_sweep_substeps"]
    tool = np.ascontiguousarray(plain._goal_tool.reshape(12))
    tgt = tool.copy()  # an orthonormal frame
    out = {}

    def note(name, rc):
        out[name] = [int(rc), (lib.edmp_last_error() or b"").decode() if rc else ""]

    set_self = lambda mask_=mask, w=sw, m=sm, n=B, T_=T: lib.edmp_sdf_set_self(h, pi(mask_), pd(w), pd(m), n, T_)  # noqa: E731
    set_goal = lambda w=gw, r=gr, k=gk, tool_=tool, tgt_=tgt, n=B: lib.edmp_sdf_set_goal(h, pd(w), pd(r), pi(k), pd(tool_), None if tgt_ is None else pd(tgt_), n)  # noqa: E731
    set_sweep = lambda w=ww, k=wk, n=B: lib.edmp_sdf_set_sweep(h, pd(w), pi(k), n)  # noqa: E731
    for name, f in (("self", set_self), ("goal", set_goal), ("sweep", set_sweep)):
        note(f"set_{name} before the sphere table", f())
    guide = build_guide(case)
    guide._bind()

    def edited(a, row, v):
        a = np.array(a, copy=True)
        a[row] = v
        return a

    bad_mask, skew = edited(mask, 5, 2), edited(tool, 0, tool[0] + 1e-4)
    nan = np.full(B, np.nan)
    for name, rc in (("set_self wrong n", lambda: set_self(n=B - 1)), ("set_self wrong T", lambda: set_self(T_=T - 1)), ("set_self T = -1", lambda: set_self(T_=-1)), ("set_self T = 0", lambda: set_self(T_=0)), ("set_self weight on an sv row", lambda: set_self(w=edited(sw, 5, 1.0))),
                     ("set_self negative margin", lambda: set_self(m=-sm - 1.0)), ("set_self NaN weight", lambda: set_self(w=nan)), ("set_self negative weight", lambda: set_self(w=-sw - 1.0)),
                     ("set_self mask entry 2", lambda: set_self(mask_=bad_mask)), ("set_self null", lambda: lib.edmp_sdf_set_self(h, None, None, None, B, T)),
                     ("set_goal wrong n", lambda: set_goal(n=B - 1)), ("set_goal weight on an sv row", lambda: set_goal(w=edited(gw, 5, 1.0))), ("set_goal NaN weight", lambda: set_goal(w=nan)),
                     ("set_goal negative rotation", lambda: set_goal(r=-gr - 1.0)), ("set_goal window 0", lambda: set_goal(k=edited(gk, 2, 0))), ("set_goal skew tool", lambda: set_goal(tool_=skew)),
                     ("set_goal target not orthonormal", lambda: set_goal(tgt_=2 * tgt)), ("set_goal NaN tool", lambda: set_goal(tool_=edited(tool, 3, np.nan))),
                     ("set_goal null", lambda: lib.edmp_sdf_set_goal(h, None, None, None, None, None, B)),
                     ("set_sweep wrong n", lambda: set_sweep(n=B - 1)), ("set_sweep weight on an sv row", lambda: set_sweep(w=edited(ww, 5, 1.0))), ("set_sweep K = 1", lambda: set_sweep(k=edited(wk, 0, 1))),
                     ("set_sweep K = 65", lambda: set_sweep(k=edited(wk, 1, 65))), ("set_sweep NaN weight", lambda: set_sweep(w=nan)), ("set_sweep negative weight", lambda: set_sweep(w=-ww - 1.0)),
                     ("set_sweep null", lambda: lib.edmp_sdf_set_sweep(h, None, None, B))):
        note(name, rc())
    # the reports: shapes, steps and rows
    Xd = ctx.to_dev(case["joints"], torch.float64)
    wide = ctx.to_dev(np.zeros((2, 7, 63)), torch.float64)
    o = ctx.empty((4, B), torch.float64)
    op = [C.c_void_p(o[i].data_ptr()) for i in range(4)]
    s7, g7 = pd(case["start"]), pd(case["goal"])
    for name, rc in (("self_rows t >= 1 on 3 rows", lambda: lib.edmp_sdf_self_rows_dev(h, ptr(Xd), 3, L, 0, L, T_CHECK, op[0], op[1])),
                     ("self_rows L = 63", lambda: lib.edmp_sdf_self_rows_dev(h, ptr(wide), 2, 63, 0, 63, 0, op[0], op[1])),
                     ("self_rows n = 0", lambda: lib.edmp_sdf_self_rows_dev(h, ptr(Xd), 0, L, 0, L, 0, op[0], op[1])),
                     ("self_rows columns outside", lambda: lib.edmp_sdf_self_rows_dev(h, ptr(Xd), B, L, 1, L, 0, op[0], op[1])),
                     ("self_rows negative off", lambda: lib.edmp_sdf_self_rows_dev(h, ptr(Xd), B, L, -1, L, 0, op[0], op[1])),
                     ("self_rows t outside", lambda: lib.edmp_sdf_self_rows_dev(h, ptr(Xd), B, L, 0, L, T + 1, op[0], op[1])),
                     ("self_rows null", lambda: lib.edmp_sdf_self_rows_dev(h, None, B, L, 0, L, 0, op[0], op[1])),
                     ("goal_rows t >= 1 on 3 rows", lambda: lib.edmp_sdf_goal_rows_dev(h, ptr(Xd), 3, L, 0, L, T_CHECK, *op)),
                     ("goal_rows L = 63", lambda: lib.edmp_sdf_goal_rows_dev(h, ptr(wide), 2, 63, 0, 63, 0, *op)),
                     ("goal_rows n = 0", lambda: lib.edmp_sdf_goal_rows_dev(h, ptr(Xd), 0, L, 0, L, 0, *op)),
                     ("goal_rows columns outside", lambda: lib.edmp_sdf_goal_rows_dev(h, ptr(Xd), B, L, 1, L, 0, *op)),
                     ("goal_rows ldw = 0", lambda: lib.edmp_sdf_goal_rows_dev(h, ptr(Xd), B, 0, 0, L, 0, *op)),
                     ("goal_rows null", lambda: lib.edmp_sdf_goal_rows_dev(h, None, B, L, 0, L, 0, *op)),
                     ("sweep_rows substeps 4 at t >= 1", lambda: lib.edmp_sdf_sweep_rows_dev(h, ptr(Xd), B, L, T_CHECK, s7, g7, 4, op[0], op[1])),
                     ("sweep_rows own substeps on 3 rows", lambda: lib.edmp_sdf_sweep_rows_dev(h, ptr(Xd), 3, L, 0, s7, g7, 0, op[0], op[1])),
                     ("sweep_rows substeps 65", lambda: lib.edmp_sdf_sweep_rows_dev(h, ptr(Xd), B, L, 0, s7, g7, 65, op[0], op[1])),
                     ("sweep_rows substeps 1", lambda: lib.edmp_sdf_sweep_rows_dev(h, ptr(Xd), B, L, 0, s7, g7, 1, op[0], op[1])),
                     ("sweep_rows L = 63", lambda: lib.edmp_sdf_sweep_rows_dev(h, ptr(wide), 2, 63, 0, s7, g7, 4, op[0], op[1]))):
        note(name, rc())
    # derived targets without a pair, and every report after a new sphere table dropped the terms
    note("set_goal derived", set_goal(tgt_=None))
    note("goal_rows derived before a pair", lib.edmp_sdf_goal_rows_dev(h, ptr(Xd), B, L, 0, L, 0, *op))
    _capi.check(lib.edmp_sdf_set(h, _capi.as_pf(guide._sdf["spheres"]), int(guide._sdf["spheres"].shape[0]), _capi.as_pi32(guide._sdf["rows"]), _capi.as_pd(guide._sdf["margin"]),
                                 _capi.as_pd(guide._sdf["smooth"]), B, T), "edmp_sdf_set")
    note("self_rows after a new table", lib.edmp_sdf_self_rows_dev(h, ptr(Xd), B, L, 0, L, 0, op[0], op[1]))
    note("goal_rows after a new table", lib.edmp_sdf_goal_rows_dev(h, ptr(Xd), B, L, 0, L, 0, *op))
    note("sweep_rows after a new table", lib.edmp_sdf_sweep_rows_dev(h, ptr(Xd), B, L, 0, s7, g7, 0, op[0], op[1]))
    ctx.bound_guide = None  # (the slot's tables are no longer what the guide object believes)
    # in a batch a message names the scene and the row inside it
    batch = SceneBatch([build_guide(case, bind=False), build_guide(case, bind=False)])
    batch._bind()
    two = lambda a, b=None: np.concatenate([a, a if b is None else b])  # noqa: E731
    note("batch set_self weight on an sv row", lib.edmp_sdf_set_self(h, pi(mask), pd(two(sw, edited(sw, 5, 1.0))), pd(two(sm)), 2 * B, T))
    note("batch set_self negative margin", lib.edmp_sdf_set_self(h, pi(mask), pd(two(sw)), pd(two(sm, edited(sm, (2, 7), -0.5))), 2 * B, T))
    note("batch set_goal weight on an sv row", lib.edmp_sdf_set_goal(h, pd(two(gw, edited(gw, 5, 1.0))), pd(two(gr)), pi(two(gk)), pd(tool), None, 2 * B))
    note("batch set_goal window 0", lib.edmp_sdf_set_goal(h, pd(two(gw)), pd(two(gr)), pi(two(gk, edited(gk, 2, 0))), pd(tool), None, 2 * B))
    note("batch set_sweep weight on an sv row", lib.edmp_sdf_set_sweep(h, pd(two(ww, edited(ww, 5, 1.0))), pi(two(wk)), 2 * B))
    note("batch set_sweep K = 65", lib.edmp_sdf_set_sweep(h, pd(two(ww)), pi(two(wk, edited(wk, 1, 65))), 2 * B))
    note("batch goal_rows on 3 rows", lib.edmp_sdf_goal_rows_dev(h, ptr(Xd), 3, L, 0, L, 0, *op))
    ctx.sync()
    return out


def gpu_record():
    return {"guide": gpu_guide_cells(), "batch": gpu_batch_cells(), "refusals": gpu_refusals()}
