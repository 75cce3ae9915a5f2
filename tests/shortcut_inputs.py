"""The shortcut stage's rule as plain Python loops, its admission check and the inputs of its tests (test infrastructure, no GPU needed).

The rule is the specification of shortcut_rows_kernel (edmp_amd/csrc/shortcut.hip; include/edmp_hip.h states it), written from the
definition with the success check's host twin as the judge - not from the kernel:

    spans    s_0 = N - 1, s_{k+1} = (s_k + 1) // 2, ending after the entry s = 2
    per pass, per span s: i = 0; while i + s <= N - 1, j = i + s:
        gain = sum_{m=i}^{j-1} |x_{m+1} - x_m| - |x_j - x_i|   (index order);  not gain > min_gain: i += 1, nothing tested
        piece  y_m = x_i + ((m - i) / (j - i)) (x_j - x_i)
        test   every configuration of the piece strictly between waypoints i and j that success_rows forms (y_m and the K - 1 interpolants
               (1 - f) y_m + f y_{m+1} of every segment), each handed to oracle.success_oracle.success_rows as a row of ONE waypoint
        no hit: x_m <- y_m, log (i, j), i = j;  hit: i += 1
    a pass that accepts nothing ends the row

A case is ADMITTED (admit) only if the rule gives the same log with every obstacle's extents grown and shrunk by 1e-6 m, with the piece
interpolated the other way ((1 - g) x_i + g x_j), and if every examined gain is more than 1e-9 away from min_gain: then no decision of
the run sits on a rounding."""
import math

import numpy as np

from edmp_amd import franka
from oracle import success_oracle as SO
from tests import repair_inputs as RI
from tests import sdf_reference as R

EXTENTS = franka.PLACEHOLDER_LINK_EXTENTS  # the link boxes of the test guides (tests/test_gpu_repair.py: make_guide)
MIN_GAIN = 1e-6
GROW = 1e-6      # metres, admission: the obstacles' extents grown and shrunk by this
GAIN_GAP = 1e-9  # admission: no examined gain closer than this to min_gain
_cache = {}


def schedule(N):
    """the spans of one pass: N - 1, then (s + 1) // 2, the last entry being 2"""
    s = N - 1
    out = [s]
    while s > 2:
        s = (s + 1) // 2
        out.append(s)
    return out


def distance(a, b):
    """|b - a| over the seven joints, squares summed in joint order, every operation rounded on its own"""
    s = 0.0
    for j in range(7):
        d = float(b[j]) - float(a[j])
        s = s + d * d
    return math.sqrt(s)


def path_length(x):
    """the joint path length of a row (7, N): the segment lengths summed in index order"""
    total = 0.0
    for m in range(x.shape[1] - 1):
        total = total + distance(x[:, m], x[:, m + 1])
    return total


def piece(x, i, j, other=False):
    """the chord's points at the columns i..j (7, j - i + 1); other: the interpolation written the other way (the yardstick)"""
    y = x[:, i:j + 1].copy()
    for m in range(i + 1, j):
        g = float(m - i) / float(j - i)
        y[:, m - i] = (1.0 - g) * x[:, i] + g * x[:, j] if other else x[:, i] + g * (x[:, j] - x[:, i])
    return y


def piece_configurations(y, K):
    """the configurations of the piece strictly between its first and last waypoint, as success_rows forms them -> (M, 7)"""
    sp = y.shape[1] - 1
    out = []
    for c in range(1, sp * K):
        m, k = divmod(c, K)
        f = float(k) / float(K)
        out.append(y[:, m].copy() if k == 0 else (1.0 - f) * y[:, m] + f * y[:, m + 1])
    return np.array(out)


def cylinder_overlap_without_cap_plane(Rb, cb, hb, Rc, cc, radius, half_height):
    """oracle.success_oracle.obb_cylinder_overlap_batch WITHOUT its last step (the face x cap-plane segments): the slab test, the axis
    line against the box and the twelve clipped box edges only.  Not a collision test - it misses a cap rim that dips into a face - but
    the tool that shows which decisions of the rule that last step alone makes (test_shortcut_host.py: test_case_conditions)"""
    R = np.einsum("...ki,...kj->...ij", Rc, Rb)
    t = np.einsum("...ki,...k->...i", Rc, cb - cc)
    hb = np.broadcast_to(hb, t.shape)
    H = np.broadcast_to(np.asarray(half_height, dtype=np.float64), t.shape[:-1])
    r2 = np.broadcast_to(np.asarray(radius, dtype=np.float64) ** 2, t.shape[:-1])
    miss = np.abs(t[..., 2]) > H + hb[..., 0] * np.abs(R[..., 2, 0]) + hb[..., 1] * np.abs(R[..., 2, 1]) + hb[..., 2] * np.abs(R[..., 2, 2])
    lo, hi = -H, H
    for i in range(3):
        lo, hi = SO._clip_b(lo, hi, -(R[..., 0, i] * t[..., 0] + R[..., 1, i] * t[..., 1] + R[..., 2, i] * t[..., 2]), R[..., 2, i], hb[..., i])
    hit = lo <= hi
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        for sj in (-1.0, 1.0):
            for sk in (-1.0, 1.0):
                p0 = t + (sj * hb[..., j])[..., None] * R[..., :, j] + (sk * hb[..., k])[..., None] * R[..., :, k] - hb[..., i][..., None] * R[..., :, i]
                d = (2.0 * hb[..., i])[..., None] * R[..., :, i]
                s0, s1 = SO._clip_b(np.zeros_like(H), np.ones_like(H), p0[..., 2], d[..., 2], H)
                d2 = SO._seg_dist2_origin_b(p0[..., 0] + s0 * d[..., 0], p0[..., 1] + s0 * d[..., 1], p0[..., 0] + s1 * d[..., 0], p0[..., 1] + s1 * d[..., 1])
                hit |= (s0 <= s1) & (d2 <= r2)
    return hit & ~miss


def any_hit(Q, obstacle_config, kinds, cap_plane=True):
    """the success check's test on each configuration of Q (M, 7): a row of one waypoint is that configuration alone.  cap_plane=False:
    the same with the cylinder test's last step left out (cylinder_overlap_without_cap_plane) - for test_case_conditions only"""
    if cap_plane:
        return bool((SO.success_rows(Q[:, :, None], obstacle_config, 1, kinds, EXTENTS)["first"] >= 0).any())
    he = franka.link_half_extents(EXTENTS).astype(np.float64)
    Rl, cl = SO.link_box_poses_batch(Q)
    Ro, co, ho, kd = SO.obstacle_shapes(obstacle_config, kinds)
    hit = False
    for o in range(len(co)):
        if kd[o] == 1:
            hit = hit or bool(cylinder_overlap_without_cap_plane(Rl, cl, he[None], Ro[o], co[o], 2 * ho[o, 0], ho[o, 2]).any())
        else:
            hit = hit or bool(SO.obb_overlap_batch(Rl, cl, he[None], Ro[o], co[o], ho[o]).any())
    return hit


def shortcut_row(x, obstacle_config, kinds, passes, K=4, min_gain=MIN_GAIN, other=False, cap_plane=True):
    """the rule on one row (7, N) -> dict(x, log [(i, j)], rejected [(i, j)], gains [every examined gain], tested, accepted, length0, length)"""
    x = np.array(x, dtype=np.float64)
    N = x.shape[1]
    if not np.isfinite(x).all():
        return dict(x=x, log=[], rejected=[], gains=[], tested=0, accepted=-1, length0=float("nan"), length=float("nan"))
    seg = [distance(x[:, m], x[:, m + 1]) for m in range(N - 1)]
    length0 = path_length(x)
    log, rejected, gains = [], [], []
    for _ in range(int(passes)):
        before = len(log)
        for s in schedule(N):
            i = 0
            while i + s <= N - 1:
                j = i + s
                total = 0.0
                for m in range(i, j):
                    total = total + seg[m]
                gain = total - distance(x[:, i], x[:, j])
                gains.append(gain)
                if not gain > min_gain:
                    i += 1
                    continue
                y = piece(x, i, j, other)
                if any_hit(piece_configurations(y, K), obstacle_config, kinds, cap_plane):
                    rejected.append((i, j))
                    i += 1
                    continue
                x[:, i:j + 1] = y
                for m in range(i, j):
                    seg[m] = distance(x[:, m], x[:, m + 1])
                log.append((i, j))
                i = j
        if len(log) == before:
            break
    return dict(x=x, log=log, rejected=rejected, gains=gains, tested=len(log) + len(rejected), accepted=len(log), length0=length0, length=path_length(x))


def shortcut_rows(X, obstacle_config, kinds, passes, K=4, min_gain=MIN_GAIN, other=False, log_cap=128, cap_plane=True):
    """the rule on every row of X (n, 7, N) -> the dict of guide.shortcut_rows plus `runs`, the per-row records"""
    runs = [shortcut_row(x, obstacle_config, kinds, passes, K, min_gain, other, cap_plane) for x in np.asarray(X, dtype=np.float64)]
    spans = np.full((len(runs), log_cap, 2), -1, dtype=np.int32)
    for r, run in enumerate(runs):
        for k, ij in enumerate(run["log"][:log_cap]):
            spans[r, k] = ij
    return dict(trajectories=np.stack([run["x"] for run in runs]), accepted=np.array([run["accepted"] for run in runs], dtype=np.int32),
                tested=np.array([run["tested"] for run in runs], dtype=np.int32), length0=np.array([run["length0"] for run in runs]),
                length=np.array([run["length"] for run in runs]), spans=spans, runs=runs)


def grown(obstacle_config, by):
    oc = np.array(obstacle_config, dtype=np.float64)
    oc[:, 7:10] += by
    return oc


def admit(X, obstacle_config, kinds, passes, K=4, min_gain=MIN_GAIN):
    """-> (admitted, reason, the rule's result): the same log with the extents grown and shrunk by GROW and with the piece interpolated the
    other way, and no examined gain within GAIN_GAP of min_gain"""
    ref = shortcut_rows(X, obstacle_config, kinds, passes, K, min_gain)
    for r, run in enumerate(ref["runs"]):
        near = [g for g in run["gains"] if abs(g - min_gain) <= GAIN_GAP]
        if near:
            return False, f"row {r}: a gain of {near[0]!r} within {GAIN_GAP} of min_gain", ref
    variants = (("the obstacles grown", grown(obstacle_config, GROW), False), ("the obstacles shrunk", grown(obstacle_config, -GROW), False),
                ("the piece interpolated the other way", obstacle_config, True))
    for what, oc, other in variants:
        alt = shortcut_rows(X, oc, kinds, passes, K, min_gain, other=other)
        for r, (a, b) in enumerate(zip(ref["runs"], alt["runs"])):
            if a["log"] != b["log"] or a["rejected"] != b["rejected"]:
                return False, f"row {r}: another log with {what}", ref
    return True, "", ref


def yardstick(X, obstacle_config, kinds, passes, K, ref):
    """what float64 itself costs on these inputs: the rule against itself with the piece interpolated the other way, with a floor of one
    ulp of the largest joint value (trajectories) / of the largest length (lengths)"""
    alt = shortcut_rows(X, obstacle_config, kinds, passes, K, other=True)
    fin = np.isfinite(ref["length0"])
    x_floor = float(np.spacing(np.abs(np.asarray(X)[fin]).max())) if fin.any() else 0.0
    l_floor = float(np.spacing(ref["length0"][fin].max())) if fin.any() else 0.0
    return dict(trajectories=max(float(np.abs(alt["trajectories"][fin] - ref["trajectories"][fin]).max()) if fin.any() else 0.0, x_floor),
                length=max(float(np.abs(alt["length"][fin] - ref["length"][fin]).max()) if fin.any() else 0.0, l_floor))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def line_state(start, goal, N):
    f = np.linspace(0.0, 1.0, N)
    X = np.ascontiguousarray((np.asarray(start)[:, None] * (1 - f) + np.asarray(goal)[:, None] * f)[None])
    X[0, :, 0], X[0, :, -1] = start, goal
    return X, f


def zigzag_rows(start, goal, N, n=1):
    """n rows (n, 7, N): the straight line minus 0.5 sin(pi f) on joint 1 plus 0.1 (-1)^w on joint 3 of the interior waypoints; row r > 0
    has its bump scaled by 1 - 0.15 r, so that the rows differ"""
    X, f = line_state(start, goal, N)
    X = np.repeat(X, n, axis=0)
    w = np.arange(N)
    for r in range(n):
        X[r, 1] -= (1.0 - 0.15 * r) * 0.5 * np.sin(np.pi * f)
        X[r, 3, 1:-1] += 0.1 * (-1.0) ** w[1:-1]
        X[r, :, 0], X[r, :, -1] = start, goal
    return np.ascontiguousarray(X)


def crowded_graze_scene(shift):
    """repair_inputs.graze_scene with 64 obstacles, cuboids first: its cube, 55 boxes >= 5 m away, then 8 cylinders of radius 0.03 m and
    height 0.06 m - seven far away and one at the tool position of joint 0 = 0.25 rad on the straight line"""
    from edmp_amd import evaluation as EV

    g = RI.graze_scene(shift)
    far = R.make_case(5, 1, 1, 63, 7, far=True)["obstacle_config"]
    q = (g["start"] + g["goal"]) / 2
    q[0] = 0.25
    tool = np.asarray(EV.end_effector_positions(q.reshape(7, 1))[0], dtype=np.float64)
    cyl = np.array([[tool[0], tool[1], tool[2], 0.0, 0.0, 0.0, 1.0, 0.03, 0.03, 0.06]])
    oc = np.concatenate([g["obstacle_config"], far[:55], far[56:], cyl])
    kinds = np.zeros(64, dtype=np.int32)
    kinds[56:] = 1
    return dict(g, obstacle_config=np.ascontiguousarray(oc), kinds=kinds)


def bumped_rows(inp, n, N, amplitude, seed):
    """n plan-like rows (n, 7, N): the straight line from start to goal plus, per row and joint, a half-sine bump of a uniform random height"""
    rs = np.random.RandomState(seed)
    X, f = line_state(inp["start"], inp["goal"], N)
    X = np.ascontiguousarray(X + rs.uniform(-amplitude, amplitude, size=(n, 7, 1)) * np.sin(np.pi * f)[None, None, :])
    X[:, :, 0], X[:, :, -1] = inp["start"], inp["goal"]
    return X


def cylinder_graze_scene(shift):
    """repair_inputs.graze_scene with a tilted cylinder of radius 0.1 m and height 0.2 m in the place of its cube"""
    g = RI.graze_scene(shift)
    oc = g["obstacle_config"].copy()
    quat = np.array([0.3, 0.2, 0.1, 0.9])
    oc[0, 3:7] = quat / np.linalg.norm(quat)
    oc[0, 7:10] = (0.1, 0.1, 0.2)
    return dict(g, obstacle_config=oc, kinds=np.ones(1, dtype=np.int32))


# ---- a candidate that the cylinder test's LAST step alone rejects ------------------------------------------------------------------------
CAP = dict(link=4, axis=0, radius=0.03, height=0.06, tilt=np.pi / 4, lift=0.01)


def cap_plane_scene(side=1.0, twist=0.0):
    """the graze scenes' start / goal (the mid configuration with joint 0 at -0.5 / +0.5 rad) and ONE cylinder whose end cap dips with its
    rim into the largest face of link box 4 at the chord's midpoint (joint 0 = 0): the cap centre sits `lift` above the face, the axis
    leaves the face tilted by `tilt` from its normal (towards the face's in-plane direction turned by `twist`), so the rim reaches
    radius x sin(tilt) - lift = 0.011 m below the face while the axis never enters the box and every box edge stays far outside the
    radius.  Only the face x cap-plane step of the cylinder test sees that contact.  side: which of the two faces along the axis"""
    g = RI.graze_scene(0.0)
    he = franka.link_half_extents(EXTENTS).astype(np.float64)
    q = (g["start"] + g["goal"]) / 2
    Rl, cl = SO.link_box_poses(q)[CAP["link"]]
    a = CAP["axis"]
    n = side * Rl[:, a]
    t1, t2 = Rl[:, (a + 1) % 3], Rl[:, (a + 2) % 3]
    t = np.cos(twist) * t1 + np.sin(twist) * t2
    zc = np.cos(CAP["tilt"]) * n + np.sin(CAP["tilt"]) * t
    xc = np.cross(zc, n)
    xc /= np.linalg.norm(xc)
    Ro = np.stack([xc, np.cross(zc, xc), zc], axis=1)
    from scipy.spatial.transform import Rotation

    cap_centre = cl + (he[CAP["link"], a] + CAP["lift"]) * n
    centre = cap_centre + (CAP["height"] / 2) * zc
    oc = np.concatenate([centre, Rotation.from_matrix(Ro).as_quat(), [CAP["radius"], CAP["radius"], CAP["height"]]])[None]
    return dict(g, obstacle_config=np.ascontiguousarray(oc), kinds=np.ones(1, dtype=np.int32))


def cap_plane_rows(g, n):
    """n rows (n, 7, 3): start, a waypoint off the chord (joint 1 lowered by 0.3 + 0.1 r rad, away from the cylinder), goal - with K = 1 the
    one candidate (0, 2) tests the chord's midpoint alone"""
    X = np.repeat(line_state(g["start"], g["goal"], 3)[0], n, axis=0)
    X[:, 1, 1] -= 0.3 + 0.1 * np.arange(n)
    return np.ascontiguousarray(X)


# name -> how the case is made; every case is admitted at its passes and K (test_shortcut_host.py checks that, case()'s assert too)
CASES = {
    "N3_o1_n5": dict(kind="random", N=3, no=1, ncyl=0, n=5, K=4, passes=2, seed=3),
    "N4_o7c2_n5": dict(kind="random", N=4, no=7, ncyl=2, n=5, K=4, passes=2, seed=1),
    "N14_graze_zigzag": dict(kind="zigzag", N=14, shift=0.0, n=1, K=4, passes=2),
    "N14_graze_zigzag_K1": dict(kind="zigzag", N=14, shift=0.04, n=1, K=1, passes=2),
    "N50_graze_zigzag": dict(kind="zigzag", N=50, shift=0.0, n=1, K=4, passes=2),
    "N64_graze_zigzag_K8_n5": dict(kind="zigzag", N=64, shift=-0.04, n=5, K=8, passes=1),
    "N14_o64c8_zigzag": dict(kind="zigzag", N=14, shift=0.0, n=2, K=4, passes=2, crowded=True),
    # the cylinder test's last step alone rejects (0, 2); the tilt direction decides whether that step swaps the face's two axes (twist 0 and
    # 3: it does not, 1 and 2: it does)
    "N3_cap_plane_K1_n5": dict(kind="cap_plane", N=3, n=5, K=1, passes=2, side=1.0, twist=0.0),
    "N3_cap_plane_K1_twist1": dict(kind="cap_plane", N=3, n=1, K=1, passes=2, side=1.0, twist=1.0),
    "N3_cap_plane_K1_twist2": dict(kind="cap_plane", N=3, n=1, K=1, passes=2, side=1.0, twist=2.0),
    "N3_cap_plane_K1_twist3": dict(kind="cap_plane", N=3, n=1, K=1, passes=2, side=-1.0, twist=3.0),
    "N14_cylinder_zigzag_n5": dict(kind="zigzag", N=14, shift=0.0, n=5, K=4, passes=2, cylinder=True),  # (every rejection is the cylinder's)
}


def make_inputs(name):
    """X, obstacle_config, kinds of a case (nothing evaluated)"""
    c = CASES[name]
    if c["kind"] == "cap_plane":
        g = cap_plane_scene(c["side"], c["twist"])
        return dict(X=cap_plane_rows(g, c["n"]), obstacle_config=g["obstacle_config"], kinds=g["kinds"])
    if c["kind"] == "zigzag":
        g = crowded_graze_scene(c["shift"]) if c.get("crowded") else cylinder_graze_scene(c["shift"]) if c.get("cylinder") else RI.graze_scene(c["shift"])
        return dict(X=zigzag_rows(g["start"], g["goal"], c["N"], c["n"]), obstacle_config=g["obstacle_config"], kinds=g["kinds"])
    inp = R.make_case(c["seed"], c["n"], c["N"] - 2, c["no"], c["ncyl"])
    return dict(X=RI.full_state(inp["joints"], inp["start"], inp["goal"]), obstacle_config=inp["obstacle_config"], kinds=inp["kinds"])


def case(name):
    """the inputs of a case with the rule's result and the yardstick; computed once and shared, callers do not modify it"""
    if name not in _cache:
        c = CASES[name]
        inp = make_inputs(name)
        ok, why, ref = admit(inp["X"], inp["obstacle_config"], inp["kinds"], c["passes"], c["K"])
        assert ok, f"{name}: not admitted: {why}"
        _cache[name] = dict(inp, name=name, K=c["K"], passes=c["passes"], ref=ref, cfgs=RI.plain_cfgs(inp["X"].shape[0]), custom=False, spheres=None,
                            yardstick=yardstick(inp["X"], inp["obstacle_config"], inp["kinds"], c["passes"], c["K"], ref))
    return _cache[name]


# ---- the property test's rows ------------------------------------------------------------------------------------------------------------------
# seed: the first of sdf_reference.make_case (7 boxes) whose straight line from start to goal collides while both ends are free, and for
# which the 32 bumped rows stay inside the joint limits and hold at least 8 free and 8 colliding rows and at least 16 rows with a rejected
# candidate under the rule (check_property_seed; the amplitude is the largest of 1.2, 0.9, 0.6 rad for which a seed below 200 does)
PROPERTY = dict(rows=32, N=14, no=7, ncyl=0, passes=2, K=4, amplitude=0.9, seed=11)


def property_inputs(seed):
    p = PROPERTY
    inp = R.make_case(seed, 1, p["N"] - 2, p["no"], p["ncyl"])
    X = bumped_rows(inp, p["rows"], p["N"], p["amplitude"], 1000 + seed)
    return dict(X=X, obstacle_config=inp["obstacle_config"], kinds=inp["kinds"], start=inp["start"], goal=inp["goal"], cfgs=RI.plain_cfgs(p["rows"]),
                custom=False, spheres=None)


def check_property_seed(seed):
    """asserts the conditions of the property case on the CPU -> the inputs with the rule's result"""
    p = PROPERTY
    inp = property_inputs(seed)
    oc, kinds = inp["obstacle_config"], inp["kinds"]
    line, _ = line_state(inp["start"], inp["goal"], p["N"])
    ends = np.stack([inp["start"], inp["goal"]])
    assert not any_hit(ends, oc, kinds), "an end collides"
    assert SO.success_rows(line, oc, p["K"], kinds, EXTENTS)["first"][0] >= 0, "the straight line is free"
    chk = SO.success_rows(inp["X"], oc, p["K"], kinds, EXTENTS)
    assert chk["within"].all(), "a row leaves the joint limits"  # (a shortcut can bring such a row back inside: `within` would change)
    free = chk["first"] < 0
    assert free.sum() >= 8 and (~free).sum() >= 8, f"{int(free.sum())} rows free"
    ref = shortcut_rows(inp["X"], oc, kinds, p["passes"], p["K"])
    assert sum(bool(run["rejected"]) for run in ref["runs"]) * 2 >= p["rows"], "fewer than half of the rows see a rejection"
    return dict(inp, free=free, ref=ref)


def property_case():
    if "property" not in _cache:
        _cache["property"] = check_property_seed(PROPERTY["seed"])
    return _cache["property"]
