"""The self-safe rule of the shortcut and blend stages as plain Python, its admission check and the inputs of its tests (test
infrastructure, no GPU needed).

The rule is the specification of shortcut_rows_kernel<true> and blend_rows_kernel<true> (edmp_amd/csrc/shortcut.hip, blend.hip;
include/edmp_hip.h states it), written from the definition - not from the kernels: the loops of shortcut_inputs.shortcut_row and
blend_inputs.blend_row with the judge

    rejected  iff  the success check's test hits (shortcut_inputs.any_hit / blend_inputs.hits)
              OR   a MASKED pair of link boxes overlaps at one of the tested configurations (oracle.success_oracle: link_box_poses_batch,
                   obb_overlap_batch - what tests/self_collision_inputs.reference decides with)

and a record of WHICH test rejected: 'obstacle', 'self' (the obstacle test passed, the self test alone rejected) or 'both'.  A zero mask
(or mask=None) is the obstacle-only rule of those two modules.

A case is ADMITTED if the two modules' own admission conditions hold under this rule (the same records with every obstacle's extents grown
and shrunk by 1e-6 m, the piece interpolated the other way, no gain within 1e-9 of min_gain / no comparison within 1e-9 relative, the
blended profile admitted by timing_inputs.admit) and if every self decision at every tested configuration is at least
self_collision_inputs.MIN_DECISION (1e-9 m) from its boundary.

Inputs.  Fold rows: a, b, c uniform in the joint limits from RandomState(3), trial after trial; the row a -> c -> b with N = 9 (five points on
each leg, c shared).  FOLD_TRIALS are three trials of 400 whose row is self-free under the default mask at K = 4 while the straight chord
a -> b is not (a seeded search found them; test_self_safe_host.py checks both properties again).  Blend probe: per trial of RandomState(5) a
corner c uniform in the joint limits, then a and b within +-1.5 rad per joint of it, clipped to the limits.  Such corners rarely fold: among
20000 trials four do at beta = 0.2 and none of them at a middle configuration alone with a free halved blend.  PROBE_TRIAL with reach
PROBE_REACH = 0.36 does: the polyline is self-free, the blend at beta = 0.36 (0.225 rad off the polyline) overlaps at k = 3 of K_b = 4 alone
(pair (1, 4) again, 0.6 mm from the decision), the blend at 0.18 (0.11 rad) is free at every k (0.7 mm)."""
import functools

import numpy as np

from edmp_amd import franka
from oracle import success_oracle as SO
from tests import blend_inputs as BI
from tests import repair_inputs as RI
from tests import self_collision_inputs as SCI
from tests import shortcut_inputs as SI
from tests import timing_inputs as TI

MIN_DECISION = SCI.MIN_DECISION
DEFAULT_MASK = franka.self_collision_pairs().astype(np.int32)
ZERO_MASK = np.zeros((9, 9), dtype=np.int32)
FOLD_PAIR = (1, 4)
FOLD_TRIALS = (97, 128, 325)
FOLD_N, FOLD_K = 9, 4
_HE = franka.link_half_extents(SI.EXTENTS).astype(np.float64)


def only(pair):
    m = ZERO_MASK.copy()
    m[pair[0], pair[1]] = 1
    return m


def without(pairs, mask=None):
    m = (DEFAULT_MASK if mask is None else np.asarray(mask, dtype=np.int32)).copy()
    for a, b in pairs:
        m[a, b] = 0
    return m


def self_test(Q, mask):
    """the masked pairs at each configuration of Q (M, 7) -> (hit (M,) bool, decision (M,) f64 = the smallest distance of a masked pair's
    separating-axis decision from its boundary, inf without a masked pair, pairs = the set of masked pairs that overlap somewhere)"""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 7)
    hit, decision, pairs = np.zeros(len(Q), dtype=bool), np.full(len(Q), np.inf), set()
    if mask is None or not np.triu(np.asarray(mask), 1).any() or len(Q) == 0:
        return hit, decision, pairs
    Rl, cl = SO.link_box_poses_batch(Q)
    for a in range(9):
        for b in range(a + 1, 9):
            if not mask[a][b]:
                continue
            h = SO.obb_overlap_batch(Rl[:, a], cl[:, a], _HE[a], Rl[:, b], cl[:, b], _HE[b])
            if h.any():
                pairs.add((a, b))
            hit |= h
            decision = np.minimum(decision, np.abs(SCI.sat_margin(Rl[:, a], cl[:, a], _HE[a], Rl[:, b], cl[:, b], _HE[b])))
    return hit, decision, pairs


def self_free(X, K, mask):
    """self_collision_inputs.reference's verdict per row of X (n, 7, N) at substeps K under mask, without its assertion -> (free (n,), decision (n,))"""
    Q = SCI.configurations(X, K)
    hit, dec, _ = self_test(Q.reshape(-1, 7), mask)
    return ~hit.reshape(Q.shape[:2]).any(axis=1), dec.reshape(Q.shape[:2]).min(axis=1)


# ---- the shortcut rule ---------------------------------------------------------------------------------------------------------------------
def shortcut_row(x, obstacle_config, kinds, passes, K=4, min_gain=SI.MIN_GAIN, mask=None, other=False):
    """shortcut_inputs.shortcut_row's loop with the judge of this module -> its dict plus verdicts [(i, j, 'accepted' | 'obstacle' | 'self' |
    'both')] in the order tested, self_rejected, decision (the smallest self decision distance at a tested configuration) and pairs"""
    x = np.array(x, dtype=np.float64)
    N = x.shape[1]
    if not np.isfinite(x).all():
        return dict(x=x, log=[], rejected=[], gains=[], verdicts=[], tested=0, accepted=-1, self_rejected=0, length0=float("nan"), length=float("nan"),
                    decision=float("inf"), pairs=set())
    seg = [SI.distance(x[:, m], x[:, m + 1]) for m in range(N - 1)]
    length0 = SI.path_length(x)
    log, rejected, gains, verdicts, decision, pairs = [], [], [], [], float("inf"), set()
    for _ in range(int(passes)):
        before = len(log)
        for s in SI.schedule(N):
            i = 0
            while i + s <= N - 1:
                j = i + s
                total = 0.0
                for m in range(i, j):
                    total = total + seg[m]
                gain = total - SI.distance(x[:, i], x[:, j])
                gains.append(gain)
                if not gain > min_gain:
                    i += 1
                    continue
                y = SI.piece(x, i, j, other)
                Q = SI.piece_configurations(y, K)
                obstacle = SI.any_hit(Q, obstacle_config, kinds)
                sh, sd, sp = self_test(Q, mask)
                decision = min(decision, float(sd.min()) if len(sd) else float("inf"))
                pairs |= sp
                if obstacle or sh.any():
                    verdicts.append((i, j, "both" if obstacle and sh.any() else "obstacle" if obstacle else "self"))
                    rejected.append((i, j))
                    i += 1
                    continue
                x[:, i:j + 1] = y
                for m in range(i, j):
                    seg[m] = SI.distance(x[:, m], x[:, m + 1])
                log.append((i, j))
                verdicts.append((i, j, "accepted"))
                i = j
        if len(log) == before:
            break
    return dict(x=x, log=log, rejected=rejected, gains=gains, verdicts=verdicts, tested=len(log) + len(rejected), accepted=len(log),
                self_rejected=sum(v[2] == "self" for v in verdicts), length0=length0, length=SI.path_length(x), decision=decision, pairs=pairs)


def shortcut_rows(X, obstacle_config, kinds, passes, K=4, min_gain=SI.MIN_GAIN, mask=None, other=False, log_cap=128):
    """the rule on every row of X (n, 7, N) -> the dict of guide.shortcut_rows(self_pairs=mask) plus `runs`.  obstacle_config / kinds may be
    per-row lists (a scene batch)"""
    per_row = isinstance(obstacle_config, list)
    runs = [shortcut_row(x, obstacle_config[r] if per_row else obstacle_config, kinds[r] if per_row else kinds, passes, K, min_gain, mask, other)
            for r, x in enumerate(np.asarray(X, dtype=np.float64))]
    spans = np.full((len(runs), log_cap, 2), -1, dtype=np.int32)
    for r, run in enumerate(runs):
        for k, ij in enumerate(run["log"][:log_cap]):
            spans[r, k] = ij
    return dict(trajectories=np.stack([run["x"] for run in runs]), accepted=np.array([run["accepted"] for run in runs], dtype=np.int32),
                tested=np.array([run["tested"] for run in runs], dtype=np.int32), self_rejected=np.array([run["self_rejected"] for run in runs], dtype=np.int32),
                length0=np.array([run["length0"] for run in runs]), length=np.array([run["length"] for run in runs]), spans=spans, runs=runs)


def admit_shortcut(X, obstacle_config, kinds, passes, K=4, mask=None, min_gain=SI.MIN_GAIN):
    """-> (admitted, reason, the rule's result): shortcut_inputs.admit's conditions on this rule's records, and every self decision at every
    tested configuration at least MIN_DECISION from its boundary"""
    ref = shortcut_rows(X, obstacle_config, kinds, passes, K, min_gain, mask)
    for r, run in enumerate(ref["runs"]):
        near = [g for g in run["gains"] if abs(g - min_gain) <= SI.GAIN_GAP]
        if near:
            return False, f"row {r}: a gain of {near[0]!r} within {SI.GAIN_GAP} of min_gain", ref
        if not run["decision"] >= MIN_DECISION:
            return False, f"row {r}: a self decision {run['decision']!r} m from its boundary", ref
    per_row = isinstance(obstacle_config, list)
    grow = lambda by: [SI.grown(o, by) for o in obstacle_config] if per_row else SI.grown(obstacle_config, by)  # noqa: E731
    for what, oc, other in (("the obstacles grown", grow(SI.GROW), False), ("the obstacles shrunk", grow(-SI.GROW), False),
                            ("the piece interpolated the other way", obstacle_config, True)):
        alt = shortcut_rows(X, oc, kinds, passes, K, min_gain, mask, other=other)
        for r, (a, b) in enumerate(zip(ref["runs"], alt["runs"])):
            if a["verdicts"] != b["verdicts"]:
                return False, f"row {r}: other verdicts with {what}", ref
            if not b["decision"] >= MIN_DECISION:
                return False, f"row {r}: a self decision {b['decision']!r} m from its boundary with {what}", ref
    return True, "", ref


def yardstick(X, obstacle_config, kinds, passes, K, mask, ref):
    """shortcut_inputs.yardstick under this rule: the rule against itself with the piece interpolated the other way, floors of one ulp"""
    alt = shortcut_rows(X, obstacle_config, kinds, passes, K, mask=mask, other=True)
    fin = np.isfinite(ref["length0"])
    x_floor = float(np.spacing(np.abs(np.asarray(X)[fin]).max())) if fin.any() else 0.0
    l_floor = float(np.spacing(ref["length0"][fin].max())) if fin.any() else 0.0
    return dict(trajectories=max(float(np.abs(alt["trajectories"][fin] - ref["trajectories"][fin]).max()) if fin.any() else 0.0, x_floor),
                length=max(float(np.abs(alt["length"][fin] - ref["length"][fin]).max()) if fin.any() else 0.0, l_floor))


# ---- the blend rule ------------------------------------------------------------------------------------------------------------------------
def blend_row(x, obstacle_config, kinds, limits, deviation, reach, Kb, H, mask=None):
    """blend_inputs.blend_row's loop with the judge of this module -> its dict plus self_hits (N,) - the tries of corner i that the obstacle
    test passed and the self test rejected -, tries = [(i, h, beta, obstacle hit per k, self hit per k)], decision and pairs"""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[1]
    vmax, amax, jump = limits
    dev = np.broadcast_to(np.asarray(deviation, dtype=np.float64), (7,))
    if not np.isfinite(x).all():
        return dict(beta=np.full(N, np.nan), code=np.full(N, -1, dtype=np.int32), halved=np.zeros(N, dtype=np.int32), self_hits=np.zeros(N, dtype=np.int32),
                    tested=0, gaps=[], tries=[], decision=float("inf"), pairs=set())
    beta, code, halved, self_hits = np.zeros(N), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    gaps, tries, pending, decision, pairs = [], [], {}, float("inf"), set()
    for i in range(1, N - 1):
        c = BI.corner_terms(x, i, vmax, amax, jump)
        if c["zp"] or c["z"] or c["flat"]:
            continue
        vm = BI._min(c["V2p"], c["V2"])
        gaps.append(BI._gap(c["J2"], vm))
        if not c["J2"] < vm:
            code[i] = 1
            continue
        b0 = float(reach)
        for j in range(7):
            if c["dl"][j] != 0.0:
                b0 = BI._min(b0, (4.0 * float(dev[j])) / c["dl"][j])
        pending[i] = (c, b0)
    tested, scale = 0, 1.0
    for h in range(H + 1):
        todo = []
        for i in sorted(pending):
            c, b0 = pending[i]
            b = b0 * scale
            gaps.append(BI._gap((2.0 * b) * c["K"], c["J2"]))
            if not (2.0 * b) * c["K"] > c["J2"]:
                code[i] = 2
                del pending[i]
                continue
            todo.append((i, b))
        if not todo:
            break
        Q = np.array([BI.blend_config(x, i, b, float(k) / float(Kb)) for i, b in todo for k in range(Kb + 1)]).reshape(-1, 7)
        hit = BI.hits(Q, obstacle_config, kinds).reshape(len(todo), Kb + 1)
        sh, sd, sp = self_test(Q, mask)
        decision = min(decision, float(sd.min()))
        pairs |= sp
        sh = sh.reshape(len(todo), Kb + 1)
        for (i, b), hk, sk in zip(todo, hit, sh):
            tested += Kb + 1
            tries.append((i, h, b, hk.copy(), sk.copy()))
            if sk.any() and not hk.any():
                self_hits[i] += 1
            if not hk.any() and not sk.any():
                code[i], beta[i], halved[i] = 3, b, h
                del pending[i]
            elif h == H:
                code[i] = 4
                del pending[i]
        scale = scale * 0.5
    return dict(beta=beta, code=code, halved=halved, self_hits=self_hits, tested=tested, gaps=gaps, tries=tries, decision=decision, pairs=pairs)


def blend_rows(X, obstacle_config, kinds, limits, deviation, reach, Kb, H, mask=None):
    """the rule for every row of X (n, 7, N): the arrays of guide.blend_rows(self_pairs=mask) plus `runs`"""
    X = np.asarray(X, dtype=np.float64)
    per_row = isinstance(obstacle_config, list)
    runs = [blend_row(x, obstacle_config[r] if per_row else obstacle_config, kinds[r] if per_row else kinds, limits, deviation, reach, Kb, H, mask)
            for r, x in enumerate(X)]
    return dict(beta=np.stack([r["beta"] for r in runs]), code=np.stack([r["code"] for r in runs]), halved=np.stack([r["halved"] for r in runs]),
                self_hits=np.stack([r["self_hits"] for r in runs]), tested=np.array([r["tested"] for r in runs], dtype=np.int32), runs=runs)


def admit_blend(X, obstacle_config, kinds, limits, deviation, reach, Kb, H, mask=None):
    """-> (admitted, reason, the rule's result): blend_inputs.admit's conditions on this rule's records (self_hits included), and every self
    decision at every tested configuration at least MIN_DECISION from its boundary"""
    ref = blend_rows(X, obstacle_config, kinds, limits, deviation, reach, Kb, H, mask)
    for r, run in enumerate(ref["runs"]):
        near = [g for g in run["gaps"] if g <= BI.GAP]
        if near:
            return False, f"row {r}: a comparison within {near[0]!r} relative", ref
        if not run["decision"] >= MIN_DECISION:
            return False, f"row {r}: a self decision {run['decision']!r} m from its boundary", ref
    per_row = isinstance(obstacle_config, list)
    for what, by in (("grown", BI.GROW), ("shrunk", -BI.GROW)):
        oc = [BI.grown(o, by) for o in obstacle_config] if per_row else BI.grown(obstacle_config, by)
        alt = blend_rows(X, oc, kinds, limits, deviation, reach, Kb, H, mask)
        if not all(np.array_equal(alt[k], ref[k]) for k in ("code", "halved", "self_hits")):
            return False, f"other codes with the obstacles {what}", ref
    for r, p in enumerate(BI.time_blended_rows(X, ref["beta"], *limits)["rows"]):
        ok, worst = TI.admit(p)
        if not ok:
            return False, f"row {r}: limit candidates {worst!r} relative apart", ref
    return True, "", ref


# ---- inputs: fold rows -----------------------------------------------------------------------------------------------------------------------
def far_scene():
    """ONE obstacle >= 5 m away: it fills the table and decides nothing"""
    return BI.far_obstacles(1, 0)


def two_leg_row(a, c, b, per_leg, per_leg2=None):
    """the row a -> c -> b (7, per_leg + per_leg2 - 1): per_leg (per_leg2, default the same) points on the two legs, c shared, the three
    configurations themselves at their columns"""
    f, g = np.linspace(0.0, 1.0, per_leg), np.linspace(0.0, 1.0, per_leg2 or per_leg)
    x = np.concatenate([a[:, None] * (1 - f) + c[:, None] * f, (c[:, None] * (1 - g) + b[:, None] * g)[:, 1:]], axis=1)
    x[:, 0], x[:, per_leg - 1], x[:, -1] = a, c, b
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def fold_triples(trials=FOLD_TRIALS):
    """(a, b, c) of the listed trials of the recipe: RandomState(3), per trial a, b, c uniform in the joint limits in that order"""
    rs = np.random.RandomState(3)
    lo, hi = franka.joint_limits()
    out = {}
    for t in range(max(trials) + 1):
        a, b, c = rs.uniform(lo, hi), rs.uniform(lo, hi), rs.uniform(lo, hi)
        if t in trials:
            out[t] = (a, b, c)
    return tuple(out[t] for t in trials)


def fold_rows(n, per_leg=5, per_leg2=None):
    """n fold rows (n, 7, per_leg + per_leg2 - 1), the trials of FOLD_TRIALS in turn"""
    tri = fold_triples()
    return np.ascontiguousarray(np.stack([two_leg_row(tri[r % len(tri)][0], tri[r % len(tri)][2], tri[r % len(tri)][1], per_leg, per_leg2) for r in range(n)]))


def chord_obstacle(row, link=4):
    """a 2 cm cube at the centre of link box `link` at the midpoint of the row's chord x_0 -> x_{N-1}: an obstacle ON the chord"""
    q = (row[:, 0] + row[:, -1]) / 2
    _, cl = SO.link_box_poses_batch(q[None])
    p = cl[0, link]
    return np.array([[p[0], p[1], p[2], 0.0, 0.0, 0.0, 1.0, 0.02, 0.02, 0.02]]), np.zeros(1, dtype=np.int32)


# name -> how the shortcut case is made (make_shortcut_inputs); every case is admitted at its passes, K and mask (shortcut_case asserts it)
SHORTCUT_CASES = {
    **{f"fold_n{n}": dict(rows=n, mask="default") for n in range(1, 10)},
    "fold_n3_only_pair": dict(rows=3, mask="only"),
    "fold_n3_without_pair": dict(rows=3, mask="without"),
    "fold_n3_zero_mask": dict(rows=3, mask="zero"),
    "fold_both_tests": dict(rows=3, mask="default", scene="chord"),
    "fold_N3": dict(rows=3, mask="default", per_leg=2),
    "fold_N64_K8": dict(rows=1, mask="default", per_leg=32, per_leg2=33, K=8, passes=1),
    "fold_crowded_o64c8": dict(rows=2, mask="default", scene="crowded"),
}
MASKS = {"default": DEFAULT_MASK, "only": only(FOLD_PAIR), "without": without([FOLD_PAIR]), "zero": ZERO_MASK}
_cache = {}


def make_shortcut_inputs(name):
    c = SHORTCUT_CASES[name]
    X = fold_rows(c["rows"], c.get("per_leg", 5), c.get("per_leg2"))
    if c.get("scene") == "chord":
        oc, kinds = chord_obstacle(X[0])
    elif c.get("scene") == "crowded":
        g = SI.crowded_graze_scene(0.0)
        oc, kinds = g["obstacle_config"], g["kinds"]
    else:
        oc, kinds = far_scene()
    return dict(X=X, obstacle_config=oc, kinds=kinds, mask=MASKS[c["mask"]], K=c.get("K", FOLD_K), passes=c.get("passes", 2))


def shortcut_case(name):
    """the inputs of a case with the rule's result and the yardstick; computed once and shared, callers do not modify it"""
    if name not in _cache:
        inp = make_shortcut_inputs(name)
        ok, why, ref = admit_shortcut(inp["X"], inp["obstacle_config"], inp["kinds"], inp["passes"], inp["K"], inp["mask"])
        assert ok, f"{name}: not admitted: {why}"
        inp["X"].setflags(write=False)
        _cache[name] = dict(inp, name=name, ref=ref, cfgs=RI.plain_cfgs(inp["X"].shape[0]),
                            yardstick=yardstick(inp["X"], inp["obstacle_config"], inp["kinds"], inp["passes"], inp["K"], inp["mask"], ref))
    return _cache[name]


def detour_rows(n=32, seed=23):
    """n rows a -> c -> b of the fold recipe (N = 9) from RandomState(seed), whatever they are: the property test's rows"""
    rs = np.random.RandomState(seed)
    lo, hi = franka.joint_limits()
    rows = []
    for _ in range(n):
        a, b, c = rs.uniform(lo, hi), rs.uniform(lo, hi), rs.uniform(lo, hi)
        rows.append(two_leg_row(a, c, b, 5))
    return np.ascontiguousarray(np.stack(rows))


# ---- inputs: the blend probe -----------------------------------------------------------------------------------------------------------------
PROBE_TRIAL, PROBE_REACH, PROBE_DEVIATION = 10691, 0.36, 0.25  # (4 x 0.25 / max |Delta| = 0.4 > reach: beta0 is the reach)


@functools.lru_cache(maxsize=None)
def probe_row():
    """the probe's row (1, 7, 3): a, c, b of PROBE_TRIAL"""
    rs = np.random.RandomState(5)
    lo, hi = franka.joint_limits()
    for _ in range(PROBE_TRIAL + 1):
        c = rs.uniform(lo, hi)
        a, b = np.clip(c + rs.uniform(-1.5, 1.5, 7), lo, hi), np.clip(c + rs.uniform(-1.5, 1.5, 7), lo, hi)
    X = np.ascontiguousarray(np.stack([a, c, b], axis=1)[None])
    X.setflags(write=False)
    return X


def probe_obstacle():
    """a 2 cm cube that the finger box reaches at the configuration u = 3/4 of the probe's blend at PROBE_REACH - the one at which the arm
    folds - 2 cm beyond the finger's centre there, away from its place at the corner waypoint (blend_inputs.middle_probe's construction).
    At K_b = 4 and 8 it is hit at that configuration alone; the halved blend clears it"""
    x = probe_row()[0]
    _, c1 = SO.link_box_poses_batch(BI.blend_config(x, 1, PROBE_REACH, 0.75)[None])
    _, c0 = SO.link_box_poses_batch(x[:, 1][None])
    v = c1[0, 8] - c0[0, 8]
    p = c1[0, 8] + 0.02 * v / np.linalg.norm(v)
    return np.array([[p[0], p[1], p[2], 0.0, 0.0, 0.0, 1.0, 0.02, 0.02, 0.02]]), np.zeros(1, dtype=np.int32)


def probe_in_walk(N=64, at=31, step=0.01, seed=9):
    """the probe's corner at the waypoints at - 1, at, at + 1 of a row (1, 7, N); before and behind it a random walk of `step` rad per joint
    and waypoint, clipped to the joint limits"""
    rs = np.random.RandomState(seed)
    lo, hi = franka.joint_limits()
    x = np.empty((7, N))
    x[:, at - 1:at + 2] = probe_row()[0]
    for m in range(at - 2, -1, -1):
        x[:, m] = np.clip(x[:, m + 1] + step * rs.standard_normal(7), lo, hi)
    for m in range(at + 2, N):
        x[:, m] = np.clip(x[:, m - 1] + step * rs.standard_normal(7), lo, hi)
    return np.ascontiguousarray(x[None])


def nan_rows():
    """four rows (4, 7, 3): the probe, a NaN row, the probe with its legs exchanged, the probe"""
    X = np.repeat(probe_row(), 4, axis=0)
    X[1, 2, 1] = np.nan
    X[2] = X[2][:, ::-1]
    return np.ascontiguousarray(X)


_BASE = dict(limits=BI.LIMITS, deviation=PROBE_DEVIATION, reach=PROBE_REACH, Kb=4, H=2, mask=DEFAULT_MASK)
BLEND_CASES = {
    "probe_middle_folds_h1_passes": dict(X=probe_row, scene=far_scene),
    "probe_H0_blocked_by_self_alone": dict(X=probe_row, scene=far_scene, H=0),
    "probe_hit_by_both": dict(X=probe_row, scene=probe_obstacle),
    "probe_zero_mask": dict(X=probe_row, scene=far_scene, mask=ZERO_MASK),
    "probe_without_pair": dict(X=probe_row, scene=far_scene, mask=without([FOLD_PAIR])),
    "two_N2_n2": dict(X=lambda: TI.coarse_rows(3, 2, 2), scene=far_scene),
    "probe_in_walk_N64_K8_H3": dict(X=probe_in_walk, scene=lambda: BI.far_obstacles(64, 8), Kb=8, H=3),
    "probe_nan_n4": dict(X=nan_rows, scene=far_scene),
}
# what the named cases must show (test_self_safe_host.py checks each on the CPU)
BLEND_EXPECT = {
    "probe_middle_folds_h1_passes": dict(code=[[0, 3, 0]], halved=[[0, 1, 0]], self_hits=[[0, 1, 0]], tested=[10]),
    "probe_H0_blocked_by_self_alone": dict(code=[[0, 4, 0]], halved=[[0, 0, 0]], self_hits=[[0, 1, 0]], tested=[5]),
    "probe_hit_by_both": dict(code=[[0, 3, 0]], halved=[[0, 1, 0]], self_hits=[[0, 0, 0]], tested=[10]),
    "probe_zero_mask": dict(code=[[0, 3, 0]], halved=[[0, 0, 0]], self_hits=[[0, 0, 0]], tested=[5]),
    "probe_without_pair": dict(code=[[0, 3, 0]], halved=[[0, 0, 0]], self_hits=[[0, 0, 0]], tested=[5]),
}


def blend_case(name):
    """a blend case with the rule's result: X, obstacle_config, kinds, limits, deviation, reach, Kb, H, mask, ref.  Built once, shared, never
    written to; every case is admitted (asserted here)"""
    key = ("blend", name)
    if key not in _cache:
        c = dict(_BASE, **BLEND_CASES[name])
        c["X"] = np.ascontiguousarray(c["X"]())
        c["obstacle_config"], c["kinds"] = c.pop("scene")()
        ok, why, ref = admit_blend(c["X"], c["obstacle_config"], c["kinds"], c["limits"], c["deviation"], c["reach"], c["Kb"], c["H"], c["mask"])
        assert ok, f"{name}: not admitted: {why}"
        c["X"].setflags(write=False)
        c.update(name=name, ref=ref, cfgs=RI.plain_cfgs(c["X"].shape[0]))
        _cache[key] = c
    return _cache[key]


def blend_call_args(c):
    """the keyword arguments of guide.blend_rows for a case (self_pairs apart)"""
    vmax, amax, jump = c["limits"]
    return dict(deviation=c["deviation"], reach=c["reach"], substeps=c["Kb"], halvings=c["H"], vmax=vmax, amax=amax, jump=jump)
