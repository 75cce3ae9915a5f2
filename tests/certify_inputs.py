"""The continuous certificate's rule as plain Python, its admission check and the inputs of its tests (test infrastructure, no GPU needed).

The rule is the specification of certify_rows_kernel (edmp_amd/csrc/certify.hip; include/edmp_hip.h states it) and of the gaps and radii
of edmp_amd/csrc/clearance.h.  The walk, the item and the row are written from the definition, not from the kernel.  The two gap functions
are NOT independent of clearance.h: the bit-for-bit comparison with tests/clearance_host needs the same operations in the same order, so
they state the header's arithmetic once more.  What holds the gaps to geometry is elsewhere and weaker - the implication gap > 0 =>
the oracle's exact test says disjoint on seeded pairs, the soundness of every verdict-0 row under the oracle's sampled check, and an upper
bound by a numerically minimised distance (SLSQP from three starts, 1e-6 m of tolerance; the distance is convex for box / box, and a
minimiser that stops early only makes that bound looser, never wrongly tight).  Scalar arithmetic in a stated order: every product and
sum is one rounded operation, sums run left to right as written.  The obstacles of a scene are the only vector axis (numpy, one entry per
obstacle, the same operations in the same order on each), so that a case costs a few seconds at most.

    radii    rho[l][j] = sum_{i=j+1..k} sqrt(a_i^2 + d_i^2) + max_c |p_l + S_l c|,  k = LINK_FRAME[l], 0 for j > k   (franka.motion_radii)
    gap      the maximum over unit axes of the separation of the projections: box_box_gap, box_cylinder_gap below
    item     (segment w, link l): L = sum_j |b_j - a_j| rho[l][j]; an in-order walk of the binary tree over the segment (walk); at the
             centre u of an interval of `size` leaves, g = min over the obstacles of gap, reach = L size / 2^(D+1):
               g - reach > margin + 1e-9   the interval is certified
               else the exact test hits     the item ends with a hit at u
               else at depth D or reach 0   one undecided interval
               else                         the interval is halved
    row      verdict 1 if any item hit, else 2 if any item counted an undecided interval, else 0; 3 for a non-finite row

A case is ADMITTED (admit) only if every comparison of the run is at least 1e-9 from its boundary - the acceptance inequality and the two
skip thresholds -, every exact overlap decision is the same with the obstacles' extents grown and shrunk by 1e-6 m, and the rule evaluated
in numpy.longdouble gives the same integers: then no decision of the run sits on a rounding."""
from fractions import Fraction

import numpy as np

from edmp_amd import franka
from oracle import success_oracle as SO
from tests import repair_inputs as RI
from tests import sdf_reference as R
from tests import shortcut_inputs as SI

EXTENTS = franka.PLACEHOLDER_LINK_EXTENTS  # the link boxes of the test guides
SAT_EPS = 1e-12          # obb_overlap's |R| + eps
EDGE_NORM2_MIN = 1e-6    # an edge axis with 1 - R[i][j]^2 below this is skipped
RADIAL_MIN = 1e-9        # the radial cylinder axis is skipped where the box centre is this close to the axis line
SLACK = 1e-9             # an interval is accepted if g - reach > margin + this
GROW = 1e-6              # metres, admission: the obstacles' extents grown and shrunk by this
NEAR = 1e-9              # admission: no comparison closer than this to its boundary
MAX_DEPTH = 10
F64, LD = np.float64, np.longdouble
_cache = {}


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------
def robot_tables(num=F64):
    """what a test guide hands the kernel: dh (7, 4) f64, the f32 static frames (9, 12) and half extents (9, 3) widened"""
    return dict(dh=franka.dh_table_f64().astype(num), sf=franka.static_frames().astype(np.float64).reshape(9, 12).astype(num),
                he=franka.link_half_extents(EXTENTS).astype(np.float64).astype(num))


def obstacle_table(obstacle_config, grow=0.0):
    """the library's (no, 16) f64 obstacle rows of an obstacle_config (no, 10) [centre, quaternion xyzw, extents]: R (9, row-major) from the
    normalised quaternion the way the library forms it, centre, half extents (extents / 2; `grow` is added to the extents first)"""
    out = np.zeros((len(obstacle_config), 16))
    for o, c in enumerate(np.asarray(obstacle_config, dtype=np.float64)):
        q = [float(v) for v in c[3:7]]
        n = float(np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))
        x, y, z, w = q[0] / n, q[1] / n, q[2] / n, q[3] / n
        x2, y2, z2, w2 = x * x, y * y, z * z, w * w
        xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
        out[o, :9] = [x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw), 2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw), 2 * (xz - yw), 2 * (yz + xw),
                      -x2 - y2 + z2 + w2]
        out[o, 9:12] = c[:3]
        out[o, 12:15] = (c[7:10] + grow) / 2
    return out


# ---- the chain, in chain.h's order -------------------------------------------------------------------------------------------------------
def interp_joint(a, b, u, num=F64):
    """the success check's interpolant: ONE fused multiply-add (1 - u) a + round(u b).  f64: formed exactly and rounded once"""
    if num is F64:
        return float(Fraction(1.0 - float(u)) * Fraction(float(a)) + Fraction(float(u) * float(b)))
    return (num(1) - num(u)) * num(a) + num(u) * num(b)


def link_pose(q, l, tab):
    """joint values q (k + 1 at least) -> the pose of link box l: (LR 3 x 3 nested lists, columns = axes, Lc 3), walked to frame k only"""
    num = tab["dh"].dtype.type
    k = int(franka.LINK_FRAME[l])
    Rm = [[num(1), num(0), num(0)], [num(0), num(1), num(0)], [num(0), num(0), num(1)]]
    o = [num(0), num(0), num(0)]
    for j in range(k + 1):
        sq, cq = np.sin(num(q[j])), np.cos(num(q[j]))
        aa, dd, ca, sa = tab["dh"][j]
        D = [[cq, -sq, num(0), aa], [sq * ca, cq * ca, -sa, -sa * dd], [sq * sa, cq * sa, ca, ca * dd]]
        Rn = [[Rm[a][0] * D[0][b] + Rm[a][1] * D[1][b] + Rm[a][2] * D[2][b] for b in range(3)] for a in range(3)]
        o = [Rm[a][0] * D[0][3] + Rm[a][1] * D[1][3] + Rm[a][2] * D[2][3] + o[a] for a in range(3)]
        Rm = Rn
    f = tab["sf"][l]
    LR = [[Rm[a][0] * f[b] + Rm[a][1] * f[4 + b] + Rm[a][2] * f[8 + b] for b in range(3)] for a in range(3)]
    Lc = [Rm[a][0] * f[3] + Rm[a][1] * f[7] + Rm[a][2] * f[11] + o[a] for a in range(3)]
    return LR, Lc


# ---- gaps: lower bounds on the distance ------------------------------------------------------------------------------------------------------
def box_box_gap(Ra, ca, ha, ob, edge_axes=True):
    """box (Ra columns = axes, ca, ha) against the boxes ob (m, 16) -> (gap (m,), the smallest |1 - R[i][j]^2 - 1e-6| met).  In
    obb_overlap's own R, A = |R| + eps, t: the six face axes, then the nine edge axes a_i x b_j divided by their norm"""
    num = ob.dtype.type
    eps = num(SAT_EPS)
    Rm = [[Ra[0][i] * ob[:, j] + Ra[1][i] * ob[:, 3 + j] + Ra[2][i] * ob[:, 6 + j] for j in range(3)] for i in range(3)]
    A = [[np.abs(Rm[i][j]) + eps for j in range(3)] for i in range(3)]
    d0, d1, d2 = ob[:, 9] - ca[0], ob[:, 10] - ca[1], ob[:, 11] - ca[2]
    t = [Ra[0][i] * d0 + Ra[1][i] * d1 + Ra[2][i] * d2 for i in range(3)]
    hb = [ob[:, 12], ob[:, 13], ob[:, 14]]
    g = np.abs(t[0]) - (ha[0] + (hb[0] * A[0][0] + hb[1] * A[0][1] + hb[2] * A[0][2]))
    for i in (1, 2):
        g = np.maximum(g, np.abs(t[i]) - (ha[i] + (hb[0] * A[i][0] + hb[1] * A[i][1] + hb[2] * A[i][2])))
    for j in range(3):
        g = np.maximum(g, np.abs(t[0] * Rm[0][j] + t[1] * Rm[1][j] + t[2] * Rm[2][j]) - ((ha[0] * A[0][j] + ha[1] * A[1][j] + ha[2] * A[2][j]) + hb[j]))
    near = np.inf
    if edge_axes:
        for i in range(3):
            i1, i2 = (i + 1) % 3, (i + 2) % 3
            for j in range(3):
                j1, j2 = (j + 1) % 3, (j + 2) % 3
                n2 = num(1) - Rm[i][j] * Rm[i][j]
                near = min(near, float(np.abs(n2 - num(EDGE_NORM2_MIN)).min()))
                ra = ha[i1] * A[i2][j] + ha[i2] * A[i1][j]
                rb = hb[j1] * A[i][j2] + hb[j2] * A[i][j1]
                skip = n2 < num(EDGE_NORM2_MIN)
                s = (np.abs(t[i2] * Rm[i1][j] - t[i1] * Rm[i2][j]) - (ra + rb)) / np.sqrt(np.where(skip, num(1), n2))
                g = np.where(skip, g, np.maximum(g, s))
    return g, near


def box_cylinder_gap(Rb, cb, hb, ob, radial=True):
    """box (Rb, cb, hb) against the cylinders ob (m, 16), the (r, r, h) row read as the exact test reads it (radius 2 ob[12], half height
    ob[14], axis = third column of the rotation) -> (gap (m,), the smallest |d - 1e-9| met): the cylinder axis, the three box normals, the
    radial direction from the axis line to the box centre"""
    num = ob.dtype.type
    d0, d1, d2 = cb[0] - ob[:, 9], cb[1] - ob[:, 10], cb[2] - ob[:, 11]
    Rm = [[ob[:, i] * Rb[0][j] + ob[:, 3 + i] * Rb[1][j] + ob[:, 6 + i] * Rb[2][j] for j in range(3)] for i in range(3)]
    t = [ob[:, i] * d0 + ob[:, 3 + i] * d1 + ob[:, 6 + i] * d2 for i in range(3)]
    H, rad = ob[:, 14], num(2) * ob[:, 12]
    g = (np.abs(t[2]) - H) - (hb[0] * np.abs(Rm[2][0]) + hb[1] * np.abs(Rm[2][1]) + hb[2] * np.abs(Rm[2][2]))
    for i in range(3):
        nz = Rm[2][i]
        ext = H * np.abs(nz) + rad * np.sqrt(np.maximum(num(0), num(1) - nz * nz))
        g = np.maximum(g, (np.abs(Rm[0][i] * t[0] + Rm[1][i] * t[1] + Rm[2][i] * t[2]) - hb[i]) - ext)
    near = np.inf
    if radial:
        d = np.sqrt(t[0] * t[0] + t[1] * t[1])
        near = float(np.abs(d - num(RADIAL_MIN)).min())
        skip = d < num(RADIAL_MIN)
        ds = np.where(skip, num(1), d)
        ux, uy = t[0] / ds, t[1] / ds
        ext = hb[0] * np.abs(ux * Rm[0][0] + uy * Rm[1][0]) + hb[1] * np.abs(ux * Rm[0][1] + uy * Rm[1][1]) + hb[2] * np.abs(ux * Rm[0][2] + uy * Rm[1][2])
        g = np.where(skip, g, np.maximum(g, (d - rad) - ext))
    return g, near


def exact_hit(LR, Lc, he, ob, kinds):
    """the success check's own test of ONE link box against the obstacle rows ob (m, 16): the oracle's box / box and box / cylinder tests"""
    if not len(ob):
        return False
    Rl, cl, hl = np.array(LR, dtype=ob.dtype), np.array(Lc, dtype=ob.dtype), np.array(he, dtype=ob.dtype)
    Ro = ob[:, :9].reshape(-1, 3, 3)
    hit = False
    box, cyl = kinds == 0, kinds == 1
    if box.any():
        hit = hit or bool(SO.obb_overlap_batch(Rl, cl, hl, Ro[box], ob[box, 9:12], ob[box, 12:15]).any())
    if cyl.any():
        hit = hit or bool(SO.obb_cylinder_overlap_batch(Rl, cl, hl, Ro[cyl], ob[cyl, 9:12], 2 * ob[cyl, 12], ob[cyl, 14]).any())
    return hit


# ---- the traversal ---------------------------------------------------------------------------------------------------------------------------
ACCEPT, HIT, NEITHER = "accept", "hit", "neither"


def walk(D, classify, reach_zero=False):
    """the in-order walk of the binary tree over one segment.  classify(un, size) -> ACCEPT / HIT / NEITHER for the interval of `size`
    leaves whose centre is un / 2^(D+1).  -> dict(visits [(un, size)], evaluations, undecided, first_undecided (un or None), hit (un or None))"""
    pos, level, visits, und, first_und, hit = 0, 0, [], 0, None, None
    for _ in range(2 ** (D + 1) - 1):  # the explicit trip bound: the nodes of the whole tree
        if pos >= 2 ** D:
            break
        size = 2 ** (D - level)
        un = 2 * pos + size
        visits.append((un, size))
        c = classify(un, size)
        if c == HIT:
            hit = un
            break
        if c == ACCEPT or level == D or reach_zero:
            if c != ACCEPT:
                und += 1
                first_und = un if first_und is None else first_und
            pos += size
            level = D - ((pos & -pos).bit_length() - 1)  # D - ctz(pos)
        else:
            level += 1
    return dict(visits=visits, evaluations=len(visits), undecided=und, first_undecided=first_und, hit=hit)


# ---- item and row ----------------------------------------------------------------------------------------------------------------------------
def certify_item(x, w, l, ob, kinds, D, margin, rho, tab, edge_axes=True, radial=True, use_reach=True, grown=None, trace=None):
    """the rule on item (segment w, link l) of the row x (7, N) -> walk's dict plus bound (min of g - reach over the accepted intervals)
    and near (the smallest distance of a comparison from its boundary).  grown: (ob grown, ob shrunk) - then `exact_agree` tells whether
    every exact decision was the same on both.  trace: a list that receives (w, l, un, g, reach) per evaluation"""
    num = tab["dh"].dtype.type
    k = int(franka.LINK_FRAME[l])
    L = num(0)
    for j in range(7):
        L = L + np.abs(num(x[j, w + 1]) - num(x[j, w])) * num(rho[l][j])
    if not use_reach:
        L = num(0)
    he = [tab["he"][l][m] for m in range(3)]
    box, cyl = ob[kinds == 0], ob[kinds == 1]
    state = dict(bound=np.inf, near=np.inf, exact_agree=True)
    thr = num(margin) + num(SLACK)

    def classify(un, size):
        u = num(un) / num(2 ** (D + 1))
        q = [interp_joint(x[j, w], x[j, w + 1], u, num) for j in range(k + 1)]
        LR, Lc = link_pose(q, l, tab)
        g = num(np.inf)
        if len(box):
            gb, near = box_box_gap(LR, Lc, he, box, edge_axes)
            g, state["near"] = min(g, gb.min()), min(state["near"], near)
        if len(cyl):
            gc, near = box_cylinder_gap(LR, Lc, he, cyl, radial)
            g, state["near"] = min(g, gc.min()), min(state["near"], near)
        reach = L * (num(size) / num(2 ** (D + 1)))
        slack = g - reach
        if trace is not None:
            trace.append((w, l, un, float(g), float(reach)))
        if np.isfinite(slack):
            state["near"] = min(state["near"], float(abs(slack - thr)))
        if slack > thr:
            state["bound"] = min(state["bound"], slack)
            return ACCEPT
        hit = exact_hit(LR, Lc, he, ob, kinds)
        if grown is not None:
            state["exact_agree"] = state["exact_agree"] and all(exact_hit(LR, Lc, he, alt, kinds) == hit for alt in grown)
        return HIT if hit else NEITHER

    out = walk(D, classify, reach_zero=bool(L == 0))
    out.update(state)
    return out


def key_of(w, un, l):
    """one integer per (segment, u, link): the lexicographic order of the triple is the integer order (un < 2^11, l < 16)"""
    return (w << 15) | (un << 4) | l


def certify_row(x, ob, kinds, D, margin, rho, tab, grown=None, **opts):
    """the rule on one row (7, N) -> dict(verdict, segment, fraction, link, evaluations, undecided, bound, near, exact_agree)"""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[1]
    if not np.isfinite(x).all():
        return dict(verdict=3, segment=-1, fraction=-1.0, link=-1, evaluations=0, undecided=0, bound=np.inf, near=np.inf, exact_agree=True)
    hits, unds, evals, nund, bound, near, agree = [], [], 0, 0, np.inf, np.inf, True
    for l in range(9):
        for w in range(N - 1):
            it = certify_item(x, w, l, ob, kinds, D, margin, rho, tab, grown=grown, **opts)
            evals += it["evaluations"]
            nund += it["undecided"]
            bound, near, agree = min(bound, it["bound"]), min(near, it["near"]), agree and it["exact_agree"]
            if it["hit"] is not None:
                hits.append(key_of(w, it["hit"], l))
            if it["first_undecided"] is not None:
                unds.append(key_of(w, it["first_undecided"], l))
    verdict = 1 if hits else 2 if nund else 0
    key = min(hits) if hits else min(unds) if nund else None
    seg, frac, link = (-1, -1.0, -1) if key is None else (key >> 15, ((key >> 4) & 0x7FF) / 2 ** (D + 1), key & 15)
    return dict(verdict=verdict, segment=seg, fraction=frac, link=link, evaluations=evals, undecided=nund, bound=float(bound), near=near, exact_agree=agree)


INT_KEYS = ("verdict", "segment", "link", "evaluations", "undecided")
KEYS = INT_KEYS + ("fraction", "bound")


def certify_rows(X, obstacle_config, kinds, D=6, margin=0.0, rho=None, num=F64, admission=False, **opts):
    """the rule on every row of X (n, 7, N) -> the dict of guide.certify_rows (without radii) plus near and exact_agree per row.  rho: the
    radii table to use, default franka.motion_radii(EXTENTS); num: the number type of the evaluation; admission: the exact decisions are
    also made with the obstacles grown and shrunk by GROW"""
    kinds = np.asarray(kinds, dtype=np.int32)
    tab = robot_tables(num)
    rho = (franka.motion_radii(EXTENTS) if rho is None else np.asarray(rho, dtype=np.float64)).astype(num)
    ob = obstacle_table(obstacle_config).astype(num)
    grown = tuple(obstacle_table(obstacle_config, g).astype(num) for g in (GROW, -GROW)) if admission else None
    runs = [certify_row(x, ob, kinds, D, margin, rho, tab, grown=grown, **opts) for x in np.asarray(X, dtype=np.float64)]
    out = {k: np.array([r[k] for r in runs], dtype=np.int32) for k in INT_KEYS}
    out.update(fraction=np.array([r["fraction"] for r in runs], dtype=np.float64), bound=np.array([r["bound"] for r in runs], dtype=np.float64),
               near=np.array([r["near"] for r in runs]), exact_agree=np.array([r["exact_agree"] for r in runs], dtype=bool))
    return out


def hit_configuration(x, segment, fraction):
    """the configuration a hit is reported at"""
    return np.array([interp_joint(x[j, segment], x[j, segment + 1], fraction) for j in range(7)])


def admit(X, obstacle_config, kinds, D, margin, rho=None):
    """-> (admitted, reason, the f64 rule's result, the longdouble rule's result)"""
    ref = certify_rows(X, obstacle_config, kinds, D, margin, rho, admission=True)
    if not (ref["near"] >= NEAR).all():
        return False, f"row {int(np.argmin(ref['near']))}: a comparison {ref['near'].min()!r} from its boundary", ref, None
    if not ref["exact_agree"].all():
        return False, f"row {int(np.argmin(ref['exact_agree']))}: an exact decision changes with the obstacles grown or shrunk", ref, None
    wide = certify_rows(X, obstacle_config, kinds, D, margin, rho, num=LD)
    for k in INT_KEYS + ("fraction",):
        if not np.array_equal(ref[k], wide[k]):
            return False, f"{k}: the longdouble rule gives {wide[k].tolist()}, float64 {ref[k].tolist()}", ref, wide
    return True, "", ref, wide


def bound_deviation(ref, wide):
    """the largest |bound(float64) - bound(longdouble)| over the rows with a finite bound (0 if there is none)"""
    fin = np.isfinite(ref["bound"]) & np.isfinite(wide["bound"])
    assert np.array_equal(np.isfinite(ref["bound"]), np.isfinite(wide["bound"]))
    return float(np.abs(ref["bound"][fin].astype(LD) - wide["bound"][fin].astype(LD)).max()) if fin.any() else 0.0


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def smooth_rows(seed, n, N, no, ncyl, amplitude=0.4, far=False):
    """n plan-like rows (the straight line from a random start to a random goal plus a half-sine bump per joint) in a random scene"""
    inp = R.make_case(seed, 1, 1, no, ncyl, far=far)
    oc = inp["obstacle_config"]
    if not far:  # the obstacles on a ring around the base, where the forearm and the hand pass: rows of every verdict, not all hit at link 0
        rs = np.random.RandomState(5000 + seed)
        ang, rad = rs.uniform(-np.pi, np.pi, no), rs.uniform(0.4, 0.8, no)
        oc[:, 0], oc[:, 1], oc[:, 2] = rad * np.cos(ang), rad * np.sin(ang), rs.uniform(0.1, 0.9, no)
        oc[:, 7:10] = rs.uniform(0.04, 0.2, size=(no, 3))
        if ncyl:
            oc[-ncyl:, 8] = oc[-ncyl:, 7]  # (r, r, h)
    return dict(X=SI.bumped_rows(inp, n, N, amplitude, 100 + seed), obstacle_config=oc, kinds=inp["kinds"])


def plate_scene(seed, cylinder=False):
    """the tunnelling scenes: a row of 3 waypoints, 1.2 rad of joint-space length per segment in a random direction from a random
    configuration, and ONE thin plate (5 cm x 5 cm x 2 mm; cylinder: a disc of radius 2.5 cm, 2 mm high) at the finger box's centre at
    u = 0.375 or 0.625 of a segment - between the configurations the success check tests at 4 substeps - in a random orientation"""
    rs = np.random.RandomState(seed)
    lo, hi = franka.joint_limits()
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.5
    x = np.zeros((7, 3))
    x[:, 0] = mid + half * rs.uniform(-1, 1, 7)
    for w in (1, 2):
        d = rs.standard_normal(7)
        x[:, w] = x[:, w - 1] + 1.2 * d / np.linalg.norm(d)
    w, u = int(rs.randint(2)), (0.375, 0.625)[int(rs.randint(2))]
    q = (1 - u) * x[:, w] + u * x[:, w + 1]
    _, c = SO.link_box_poses(q)[8]
    quat = rs.standard_normal(4)
    dims = (0.025, 0.025, 0.002) if cylinder else (0.05, 0.05, 0.002)
    oc = np.array([[c[0], c[1], c[2], *(quat / np.linalg.norm(quat)), *dims]])
    return dict(X=np.ascontiguousarray(x[None]), obstacle_config=oc, kinds=np.full(1, int(cylinder), dtype=np.int32), segment=w, fraction=u)


def special_rows():
    """five rows of N = 5 in the graze scene (a 6 cm cube at the tool's position of joint 0 = 0): the straight line through the cube; the
    same with its second waypoint repeated (a zero-length segment); a row that does not move, away from the cube; a NaN row; a row whose
    path is lifted off the cube except for its middle waypoint, which stays inside it (a hit at a waypoint: no interval's centre IS a
    waypoint, the walk halves towards it until a centre lies in the cube)"""
    g = RI.graze_scene(0.0)
    line = SI.line_state(g["start"], g["goal"], 5)[0][0]
    X = np.repeat(line[None], 5, axis=0)
    X[1, :, 2] = X[1, :, 1]
    X[2] = g["start"][:, None]
    X[3, 4, 2] = np.nan
    X[4] = line
    X[4, 1, 1:4] -= 0.4
    X[4, :, 2] = line[:, 2]  # the middle waypoint stays inside the cube
    return dict(X=np.ascontiguousarray(X), obstacle_config=g["obstacle_config"], kinds=g["kinds"])


def graze_rows(shift, n=1, N=3):
    """the straight line of the graze scene with the cube shifted radially by `shift`: the hand passes the cube at a small distance"""
    g = RI.graze_scene(shift)
    X = np.repeat(SI.line_state(g["start"], g["goal"], N)[0], n, axis=0)
    return dict(X=np.ascontiguousarray(X), obstacle_config=g["obstacle_config"], kinds=g["kinds"])


# name -> how the case is made; every case is admitted at its depth and margin (test_certify_host.py checks that, case()'s assert too)
CASES = {
    "N2_o1_n8": dict(kind="smooth", seed=1, n=8, N=2, no=1, ncyl=0, D=6, margin=0.0),
    "N3_o5_n2": dict(kind="smooth", seed=1, n=2, N=3, no=5, ncyl=0, D=6, margin=0.0),
    "N9_o7c2_n3_D1": dict(kind="smooth", seed=2, n=3, N=9, no=7, ncyl=2, D=1, margin=0.0),
    "N9_o7c2_n4_D0": dict(kind="smooth", seed=1, n=4, N=9, no=7, ncyl=2, D=0, margin=0.0),
    "N14_o7c2_n5_margin": dict(kind="smooth", seed=1, n=5, N=14, no=7, ncyl=2, D=6, margin=0.02),
    "N14_o5_n9": dict(kind="smooth", seed=3, n=9, N=14, no=5, ncyl=0, D=6, margin=0.0, amplitude=0.3),
    "N64_o7_n2": dict(kind="smooth", seed=6, n=2, N=64, no=7, ncyl=0, D=6, margin=0.0, amplitude=0.3),
    "N3_o64c8_n6": dict(kind="smooth", seed=1, n=6, N=3, no=64, ncyl=8, D=6, margin=0.0),
    "N3_o3c1_n3_D10": dict(kind="smooth", seed=6, n=3, N=3, no=3, ncyl=1, D=10, margin=0.0, amplitude=0.3),
    "N3_far_n7": dict(kind="smooth", seed=9, n=7, N=3, no=7, ncyl=2, D=6, margin=0.02, far=True),
    "N5_special": dict(kind="special", D=6, margin=0.0),
    "N3_graze_undecided_D2": dict(kind="graze", shift=0.08, D=2, margin=0.0),
    "N3_graze_free_D4": dict(kind="graze", shift=0.1, D=4, margin=0.0),
    "plate_box": dict(kind="plate", seed=0, cylinder=False, D=6, margin=0.0),
    "plate_cylinder": dict(kind="plate", seed=51, cylinder=True, D=6, margin=0.0),
    "plate_box_D10": dict(kind="plate", seed=20, cylinder=False, D=10, margin=0.0),
}


def make_inputs(name):
    """X, obstacle_config, kinds of a case (nothing evaluated)"""
    c = CASES[name]
    if c["kind"] == "smooth":
        return smooth_rows(c["seed"], c["n"], c["N"], c["no"], c["ncyl"], c.get("amplitude", 0.4), c.get("far", False))
    if c["kind"] == "special":
        return special_rows()
    if c["kind"] == "graze":
        return graze_rows(c["shift"])
    return plate_scene(c["seed"], c["cylinder"])


def case(name):
    """the inputs of a case with the rule's result in float64 and longdouble; computed once and shared, callers do not modify it"""
    if name not in _cache:
        c = CASES[name]
        inp = make_inputs(name)
        ok, why, ref, wide = admit(inp["X"], inp["obstacle_config"], inp["kinds"], c["D"], c["margin"])
        assert ok, f"{name}: not admitted: {why}"
        _cache[name] = dict(inp, name=name, D=c["D"], margin=c["margin"], ref=ref, wide=wide, deviation=bound_deviation(ref, wide),
                            cfgs=RI.plain_cfgs(inp["X"].shape[0]))
    return _cache[name]
