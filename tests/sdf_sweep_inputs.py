"""Checker of the swept-clearance term of the sphere signed-distance guide (sdf_sweep_kernel, edmp_amd/csrc/sdf.hip), written from the
definition - not from the kernel (test infrastructure, no GPU needed):

    q(w, k)  = (1 - f) q_w + f q_{w+1},  f = k / K,  w = 0..L,  k = 1..K-1       the success check's interpolation over the padded chain
    sweep(r) = weight_r * sum_w sum_k sum_s max(0, m_r - d(q(w, k), s))         d = the obstacle part's clearance (sdf_reference.evaluate)

The interpolants of a row are handed to `sdf_reference.evaluate` as a trajectory of (L + 1)(K - 1) columns (its hinge sum over them IS
the bare term) and its autograd gradient is carried back to the interior waypoints by the (1 - f, f) weights of the interpolation;
tests/test_sdf_sweep_host.py holds that gradient to central differences of the cost.  dtype=torch.float32 forms the interpolants in
float32 as well: the yardstick of what float32 costs on the same inputs.  `sweep_margins` is sdf_reference.margins over the interpolants
(every one of them is an "interior column" of the call above); check_case asserts them AND the waypoints' own margins >= MIN_GAP, at
t = 0 and at T_CHECK, so no element is excluded from any comparison."""
import numpy as np
import torch

from edmp_amd import franka
from tests import sdf_reference as R

T, T_CHECK, MIN_GAP = R.T, R.T_CHECK, R.MIN_GAP
# one row per guide: two weighted SDF rows (with and without grad_norm), iv and sv rows with and without it, a plain SDF row
ROW_GUIDES = R.ROW_GUIDES + (("sdf", False, 0.02),)
B = len(ROW_GUIDES)
SWEEP_ROWS = (0, 1)
SDF_ROWS = (0, 1, 6)
SWEEP_WEIGHT = (1.0, 0.75)  # of rows 0 and 1
UNBOUND_ROWS = 3  # the report with substeps= is asked for this many rows (not the bound count)


def interpolants(joints, start, goal, K, dtype=np.float64):
    """joints (n, 7, L) -> (n, 7, (L + 1)(K - 1)): column w (K - 1) + k - 1 = q(w, k), formed in `dtype`"""
    x = np.asarray(joints, dtype=np.float64).astype(dtype)
    n, _, L = x.shape
    s = np.broadcast_to(np.asarray(start, dtype=np.float64).astype(dtype).reshape(1, 7, 1), (n, 7, 1))
    g = np.broadcast_to(np.asarray(goal, dtype=np.float64).astype(dtype).reshape(1, 7, 1), (n, 7, 1))
    q = np.concatenate([s, x, g], axis=2)  # (n, 7, L + 2)
    f = (np.arange(1, K, dtype=dtype) / dtype(K)).astype(dtype)  # (K - 1,)
    out = (dtype(1) - f) * q[:, :, :-1, None] + f * q[:, :, 1:, None]  # (n, 7, L + 1, K - 1)
    return np.ascontiguousarray(out.reshape(n, 7, (L + 1) * (K - 1)).astype(dtype))


def evaluate_sweep(joints, start, goal, obstacle_config, kinds, spheres, margin, weight, K, dtype=torch.float64, want_grad=True):
    """joints (n, 7, L), margin / weight (n,), K one int or (n,) ints (rows with K < 2 or weight 0: cost 0; K < 2: clearance +inf).
    Returns f64 ndarrays cost (n,), clearance (n,) = min over the interpolants and spheres of d, grad (n, 7, L) with respect to the
    interior waypoints, coord_max, and per row the sdf_reference.evaluate result on its interpolants (`ev`, None without one)."""
    x = np.asarray(joints, dtype=np.float64)
    n, _, L = x.shape
    Ks = np.broadcast_to(np.asarray(K), (n,)).astype(int)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    cost, clr, grad, evs, cmax = np.zeros(n), np.full(n, np.inf), np.zeros((n, 7, L)), [], 0.0
    for r in range(n):
        k = int(Ks[r])
        if k < 2:
            evs.append(None)
            continue
        Q = interpolants(x[r:r + 1], start, goal, k, npdt)
        ev = R.evaluate(Q, start, goal, obstacle_config, kinds, spheres, np.asarray(margin, dtype=np.float64)[r:r + 1], np.zeros(1), dtype=dtype,
                        want_grad=want_grad)
        evs.append(ev)
        cmax = max(cmax, ev["coord_max"])
        cost[r] = float(weight[r]) * float(ev["collision"][0])
        clr[r] = float(ev["d"][0, 1:-1].min())  # (columns 0 and -1 of the call are start and goal themselves)
        if want_grad:
            gq = ev["grad"][0].reshape(7, L + 1, k - 1)
            f = np.arange(1, k, dtype=np.float64) / k
            full = np.zeros((7, L + 2))
            full[:, :-1] += (gq * (1.0 - f)).sum(-1)  # to waypoint w
            full[:, 1:] += (gq * f).sum(-1)           # to waypoint w + 1
            grad[r] = float(weight[r]) * full[:, 1:-1]  # what would land on start or goal is dropped
    return dict(cost=cost, clearance=clr, grad=grad, ev=evs, coord_max=cmax, K=Ks, L=L)


def sweep_margins(sw):
    """sdf_reference.margins over the interpolants of every row that has some: the smallest of each kind, and the largest active share"""
    out = dict(hinge=np.inf, obstacle=np.inf, axis=np.inf, rho=np.inf, active=0.0)
    for ev in sw["ev"]:
        if ev is None:
            continue
        mg = R.margins(ev)
        for k in ("hinge", "obstacle", "axis", "rho"):
            out[k] = min(out[k], mg[k])
        out["active"] = max(out["active"], mg["active"])
    return out


def assert_sweep_margins(sw, what=""):
    mg = sweep_margins(sw)
    for k in ("hinge", "obstacle", "axis", "rho"):
        assert mg[k] >= MIN_GAP, f"{what}: an interpolant sits {mg[k]:.3e} m from a decision boundary ({k}); pick another seed"
    return mg


def mixed_cfgs(spec, with_term=True, grad_norm=None):
    """the 7-row ensemble of ROW_GUIDES with the swept-clearance term on rows 0 and 1 (weights SWEEP_WEIGHT, substeps K[0], K[1]), spec
    being K or a case that holds it; with_term=False: the same rows without it (no sweep keys); grad_norm=False: no row normalises"""
    K = spec["K"] if isinstance(spec, dict) else spec
    return R.mixed_ensemble([(m, gn, lam, dict(sweep_weight=float(SWEEP_WEIGHT[i]), sweep_substeps=int(K[i])) if with_term and i in SWEEP_ROWS else None)
                             for i, (m, gn, lam) in enumerate(ROW_GUIDES)], 300, grad_norm)


# name -> L, obstacles, true cylinders among them, sphere table, substeps of rows 0 and 1, seed of sdf_reference.make_case(seed, B, ...)
# (searched with R.find_seed(lambda s: check_case(name, s)))
CASES = {
    "L1_o1_custom_K2": dict(L=1, no=1, ncyl=0, spheres="custom", K=(2, 2), seed=15),
    "L2_o7c2_default_K4": dict(L=2, no=7, ncyl=2, spheres="default", K=(4, 4), seed=0),
    "L5_o64_custom_K42": dict(L=5, no=64, ncyl=0, spheres="custom", K=(4, 2), seed=0),
    "L48_o7c2_custom_K4": dict(L=48, no=7, ncyl=2, spheres="custom", K=(4, 4), seed=2),
    "L48_o64_default_K42": dict(L=48, no=64, ncyl=0, spheres="default", K=(4, 2), seed=1324),
    "L62_o7c2_default_K8": dict(L=62, no=7, ncyl=2, spheres="default", K=(8, 8), seed=85),
}
_cache = {}


@R.cached_case(CASES)
def check_case(name, seed):
    """inputs of a case with the checkers' float64 results - obstacle part at the waypoints (sdf_reference.evaluate) and the sweep term -
    at t = 0 and at T_CHECK; asserts the distance of the waypoints AND of all interpolants from every decision boundary for both, and
    that the term's gradient is non-zero on the weighted rows at T_CHECK.  `every0`: weight 1 and K[0] on the first UNBOUND_ROWS rows at
    t = 0 (the report with substeps= on rows that are not the bound ones).  Computed once per case and shared; callers do not modify it."""
    c = CASES[name]
    cfgs = mixed_cfgs(c["K"])
    assert cfgs["total_batch_size"] == B
    what = f"{name} seed {seed}"
    inp, sph, args, sdf0, _, sdft, _ = R.obstacle_part(what, seed, cfgs, c["L"], c["no"], c["ncyl"], c["spheres"])
    mt, w, Ks = cfgs["sdf_margin"][:, T_CHECK - 1], cfgs["sdf_sweep_weight"], cfgs["sdf_sweep_substeps"]
    n = UNBOUND_ROWS
    every0 = evaluate_sweep(inp["joints"][:n], *args[1:], np.zeros(n), np.ones(n), c["K"][0], want_grad=False)
    mg_every = assert_sweep_margins(every0, f"{what} t=0, every row")
    sweep0 = evaluate_sweep(*args, np.zeros(B), w, Ks)
    mg0 = assert_sweep_margins(sweep0, f"{what} t=0")
    sweept = evaluate_sweep(*args, mt, w, Ks)
    mgt = assert_sweep_margins(sweept, f"{what} t={T_CHECK}")
    assert all(np.abs(sweept["grad"][r]).max() > 0 for r in SWEEP_ROWS), f"{what}: a weighted row has a zero sweep gradient"
    assert not sweept["grad"][[r for r in range(B) if r not in SWEEP_ROWS]].any() and not sweept["cost"][[r for r in range(B) if r not in SWEEP_ROWS]].any()
    return dict(inp, name=name, spheres=sph, custom=c["spheres"] == "custom", cfgs=cfgs, L=c["L"], K=c["K"], seed=seed, args=args, sdf0=sdf0, sdft=sdft,
                sweep0=sweep0, sweept=sweept, every0=every0, margins0=mg0, marginst=mgt, margins_every=mg_every)


def yardstick(case, t):
    """deviation of the same formulas in CPU float32 (interpolation included) from float64: the sweep cost relative to the largest, the
    minimum swept clearance absolute, and at T_CHECK the whole gradient of the weighted rows relative to its largest element"""
    cfgs = case["cfgs"]
    m = np.zeros(B) if t == 0 else cfgs["sdf_margin"][:, t - 1]
    ev = case["sweep0"] if t == 0 else case["sweept"]
    e32 = evaluate_sweep(*case["args"], m, cfgs["sdf_sweep_weight"], cfgs["sdf_sweep_substeps"], dtype=torch.float32)
    fin = np.isfinite(ev["clearance"])
    out = dict(cost=float(np.abs(e32["cost"] - ev["cost"]).max() / max(np.abs(ev["cost"]).max(), 1e-300)),
               clearance_abs=float(np.abs(e32["clearance"][fin] - ev["clearance"][fin]).max()))
    if t:
        s32 = R.evaluate(*case["args"], m, cfgs["smoothness"], dtype=torch.float32)
        rows = list(SWEEP_ROWS)
        ref = R.total_gradient(case, "sweep", SDF_ROWS)[rows]
        out["grad"] = float(np.abs(s32["grad"][rows] + e32["grad"][rows] - ref).max() / np.abs(ref).max())
    return out


# ---- the plate: positive clearance at every waypoint, a link swept through a thin obstacle between two of them ------------------------
PLATE_MARGIN = 0.035  # below the smallest waypoint clearance (+0.077 m): guide 101's hinge is silent on the row
PLATE_K = 2          # the segment's midpoint


def plate_case():
    """joint 0 from -0.4 to +0.4 rad at the mid configuration, L = 2, start = q_1, goal = q_2, one 0.12 x 0.002 x 0.12 cuboid at the
    tool's position at joint 0 = 0, default spheres.  Asserts the checker's own values: smallest waypoint clearance +0.077 m, clearance
    at the segment's midpoint -0.048 m, every kink >= 7e-3 m away."""
    if "plate" in _cache:
        return _cache["plate"]
    from edmp_amd import evaluation as EV

    lo, hi = franka.joint_limits()
    mid = (lo + hi) / 2
    q1, q2, qm = mid.copy(), mid.copy(), mid.copy()
    q1[0], q2[0], qm[0] = -0.4, 0.4, 0.0
    tool = EV.end_effector_positions(qm.reshape(7, 1))[0]
    oc = np.array([[tool[0], tool[1], tool[2], 0.0, 0.0, 0.0, 1.0, 0.12, 0.002, 0.12]])
    kinds = np.zeros(1, dtype=np.int32)
    joints = np.stack([q1, q2], axis=1)[None]  # (1, 7, 2)
    sph = R.case_spheres("default")
    args = (joints, q1, q2, oc, kinds, sph)
    way0 = R.evaluate(*args, np.zeros(1), np.zeros(1), want_grad=False)
    way = R.evaluate(*args, np.full(1, PLATE_MARGIN), np.zeros(1))
    sw0 = evaluate_sweep(*args, np.zeros(1), np.ones(1), PLATE_K, want_grad=False)
    sw = evaluate_sweep(*args, np.full(1, PLATE_MARGIN), np.ones(1), PLATE_K)
    assert abs(way0["clearance"][0] - 0.077) < 1e-3 and abs(sw0["clearance"][0] + 0.048) < 1e-3, (way0["clearance"], sw0["clearance"])
    for ev in (way0, way, sw0["ev"][0], sw["ev"][0]):
        mg = R.margins(ev)
        assert min(mg["hinge"], mg["obstacle"], mg["axis"], mg["rho"]) >= 7e-3, mg
    assert not way["grad"].any() and np.abs(sw["grad"]).max() > 0
    # a second row that rests at the midpoint, inside the plate: its waypoint hinge is active, so the batch's ||g|| is never 0 (the mix
    # of guide.hip divides by it, as the reference does)
    helper = np.stack([qm, qm], axis=1)[None]
    hev = R.evaluate(helper, q1, q2, oc, kinds, sph, np.full(1, PLATE_MARGIN), np.zeros(1))
    assert R.margins(hev)["hinge"] >= 7e-3 and np.abs(hev["grad"]).max() > 0
    out = dict(joints=joints, joints2=np.concatenate([joints, helper]), start=q1, goal=q2, obstacle_config=oc, kinds=kinds, spheres=sph, args=args, way0=way0,
               way=way, sweep0=sw0, sweep=sw)
    _cache["plate"] = out
    return out


def plate_cfgs(sweep):
    """two SDF rows (plate_case's joints2) with the constant margin PLATE_MARGIN and no smoothness; sweep=True adds weight 1 at PLATE_K
    substeps to row 0"""
    from edmp_amd import guide_cfg as GC

    d = [R.guide_dict("sdf", False, 0.0, 400), R.guide_dict("sdf", False, 0.0, 402)]
    for g in d:
        g["hyperparameters"]["sdf"]["margin"] = [PLATE_MARGIN, PLATE_MARGIN]
    if sweep:
        d[0]["hyperparameters"]["sdf"].update(sweep_weight=1.0, sweep_substeps=PLATE_K)
    return GC.build_guide_cfgs(d, 1, T)


# ---- ends: an obstacle that only the start -> q_1 segment comes near ------------------------------------------------------------------
def ends_case():
    """L = 3, K = 4, one row: the waypoints and the goal sit at the mid configuration, the start has joint 0 turned by 0.8 rad, and a
    small cube lies at the tool's position at joint 0 = 0.4 rad turned (the middle of the first segment), out of reach of the hinge
    from every waypoint: only segment 0 is active, and its first-set part would land on the start"""
    if "ends" in _cache:
        return _cache["ends"]
    from edmp_amd import evaluation as EV

    lo, hi = franka.joint_limits()
    mid = (lo + hi) / 2
    start, qh = mid.copy(), mid.copy()
    start[0], qh[0] = 0.8, 0.4
    tool = EV.end_effector_positions(qh.reshape(7, 1))[0]
    oc = np.array([[tool[0], tool[1], tool[2], 0.0, 0.0, 0.0, 1.0, 0.04, 0.04, 0.04]])
    kinds = np.zeros(1, dtype=np.int32)
    joints = np.repeat(mid.reshape(1, 7, 1), 3, axis=2)
    sph = R.case_spheres("default")
    args = (joints, start, mid, oc, kinds, sph)
    sw = evaluate_sweep(*args, np.zeros(1), np.ones(1), 4)
    way = R.evaluate(*args, np.zeros(1), np.zeros(1))
    assert_sweep_margins(sw, "ends")
    R.assert_margins(way, "ends")
    assert not way["grad"].any() and np.abs(sw["grad"][0, :, 0]).max() > 0 and not sw["grad"][0, :, 1:].any(), sw["grad"]
    out = dict(joints=joints, start=start, goal=mid.copy(), obstacle_config=oc, kinds=kinds, spheres=sph, args=args, sweep=sw)
    _cache["ends"] = out
    return out


def ends_cfgs():
    from edmp_amd import guide_cfg as GC

    d = R.guide_dict("sdf", False, 0.0, 401)
    d["hyperparameters"]["sdf"].update(margin=[0.0, 0.0], sweep_weight=1.0, sweep_substeps=4)
    return GC.build_guide_cfgs([d], 1, T)
