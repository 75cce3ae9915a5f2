"""CPU: the cases of tests/overlap_inputs.py - every tabled case rebuilds into its class, lands on its side of an independent truth, rests
on its step (the rule without that step flips it and no other case), and the table meets its caps.  The GPU runs the same cases in
tests/test_gpu_overlap.py."""
import collections

import numpy as np

from oracle import success_oracle as SO
from tests import overlap_inputs as OI
from tests import self_collision_inputs as SCI
from tests import shortcut_inputs as SI

LINK, SELF = OI.link_cases(), OI.self_cases()


def pair_of(case):
    """the two shapes of a case: (Ra, ca, ha), (Rb, cb, hb or (radius, half height))"""
    poses = SO.link_box_poses(case["q"])
    if case["kind"] < 0:
        a, b = case["pair"]
        return (poses[a][0], poses[a][1], OI.HE[a]), (poses[b][0], poses[b][1], OI.HE[b])
    l = case["link"]
    return (poses[l][0], poses[l][1], OI.HE[l]), OI.obstacle_shape(case["oc"], case["kind"])


def rule(case, **kw):
    A, B = pair_of(case)
    if case["kind"] == 1:
        return OI.cylinder_rule(*A, B[0], B[1], *B[2], **kw)
    return OI.box_rule(*A, *B, **kw)


def row_hit(case, q):
    """oracle.success_oracle.success_rows on the constant row of q against the case's one obstacle"""
    res = SO.success_rows(OI.constant_row(q)[None], np.asarray(case["oc"])[None], 1, np.array([case["kind"]], dtype=np.int32), OI.EXTENTS)
    assert res["within"][0] and bool(res["ok"][0]) == (res["first"][0] < 0) and res["first"][0] in (-1, 0)
    return bool(res["first"][0] == 0)


def test_every_case_rebuilds_into_its_class():
    assert len({c["name"] for c in LINK + SELF}) == len(LINK + SELF)
    for case in LINK + SELF:
        name, clear, verdict = OI.classify(case)
        A, B = pair_of(case)
        if case["family"] == "ZEROS":
            R = B[0].T @ A[0]
            assert R[2, 0] == 0.0 and R[2, 1] == 0.0 and R[2, 2] == 1.0, (case["name"], R[2])  # the `nj == 0` skip and the `d == 0` clip
            assert case["q"][0] == 0.0 and name == ("" if case["hit"] else "CYL_MISS")
        else:
            assert name == case["cls"], (case["name"], name)
        assert clear and OI.in_limits(case["q"]) and verdict == case["hit"], case["name"]
        if case["kind"] < 0:
            assert SO.obb_overlap(*A, *B) == case["hit"], case["name"]
        else:
            scalar = SO.obb_cylinder_overlap(*A, B[0], B[1], *B[2]) if case["kind"] == 1 else SO.obb_overlap(*A, *B)
            assert scalar == case["hit"] and row_hit(case, case["q"]) == case["hit"], case["name"]
            assert rule(case) == case["hit"]  # (the test-side copy, nothing left out, is the rule)


def test_the_other_links_decide_nothing():
    """a link case without its own link box: the obstacle grown by CLEAR touches no other box (the admission), so the eight others alone
    give a free row"""
    for case in LINK:
        poses = SO.link_box_poses(case["q"])
        Ro, co, shape = OI.obstacle_shape(case["oc"], case["kind"])
        for m in range(9):
            if m == case["link"]:
                continue
            if case["kind"] == 1:
                assert not SO.obb_cylinder_overlap(poses[m][0], poses[m][1], OI.HE[m], Ro, co, shape[0] + OI.CLEAR, shape[1] + OI.CLEAR), (case["name"], m)
            else:
                assert not SO.obb_overlap(poses[m][0], poses[m][1], OI.HE[m], Ro, co, shape + OI.CLEAR), (case["name"], m)


def test_self_cases_against_the_self_collision_reference():
    for case in SELF:
        a, b = case["pair"]
        mask = np.zeros((9, 9), dtype=bool)
        mask[a, b] = True
        ref = SCI.reference(OI.constant_row(case["q"])[None], 1, mask)
        assert ref["first"][0] == (0 if case["hit"] else -1) and ref["pair"][0].tolist() == ([a, b] if case["hit"] else [-1, -1]), case["name"]
        assert ref["decision"][0] >= OI.M  # (sat_margin of that module: the deciding axis is at least M from flipping)


# ---- independent truth ---------------------------------------------------------------------------------------------------------------------
def linf_distance(A, B, shift=None):
    """min over x in box A, y in box B (moved by `shift`) of |x - y|_inf, a linear programme in the boxes' own coordinates; metres.  The
    Euclidean distance is at least this."""
    from scipy.optimize import linprog

    (Ra, ca, ha), (Rb, cb, hb) = A, B
    k = 1e3  # millimetres: the solver's tolerances are absolute
    d = (ca - cb - (0.0 if shift is None else shift)) * k
    rows = np.concatenate([np.concatenate([Ra, -Rb, -np.ones((3, 1))], axis=1), np.concatenate([-Ra, Rb, -np.ones((3, 1))], axis=1)])
    res = linprog(np.array([0, 0, 0, 0, 0, 0, 1.0]), A_ub=rows, b_ub=np.concatenate([-d, d]),
                  bounds=[(-h * k, h * k) for h in ha] + [(-h * k, h * k) for h in hb] + [(0, None)], method="highs")
    assert res.status == 0, res.message
    return res.fun / k


def test_boxes_land_on_their_side_of_a_linear_programme():
    """SEP: the boxes are at least M / 2 apart (their L-infinity distance, a lower bound of the Euclidean one, is).  TIGHT: box B moved by
    any corner of the cube of half side M / 2 - which holds the ball of radius M / 2 - still meets box A, and the set of such moves is
    convex: the boxes overlap by at least M / 2 in every direction"""
    corners = [np.array([sx, sy, sz]) * (OI.M / 2) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    n = collections.Counter()
    for case in LINK + SELF:
        if case["kind"] == 1:
            continue
        A, B = pair_of(case)
        if case["hit"]:
            assert all(linf_distance(A, B, c) <= 1e-9 for c in corners), case["name"]
        else:
            assert linf_distance(A, B) >= OI.M / 2, case["name"]
        n[case["hit"]] += 1
    assert n[True] >= 45 and n[False] >= 45, n


def test_cylinders_land_on_their_side_of_a_numerical_minimisation():
    """the distance from the cylinder's axis to (box ∩ slab) by SLSQP (test_success_oracle.py's yardstick): at least M / 2 on the class's side"""
    n = collections.Counter()
    for case in LINK:
        if case["kind"] != 1:
            continue
        A, (Ro, co, (rad, H)) = pair_of(case)
        d = OI.axis_distance_numeric(*A, Ro, co, H)
        assert d is not None, case["name"]  # (every class has the box inside the slab)
        assert (d <= rad - OI.M / 2) if case["hit"] else (d >= rad + OI.M / 2), (case["name"], d, rad)
        n[case["hit"]] += 1
    assert n[True] >= 40 and n[False] >= 5, n


# ---- every case rests on its step -----------------------------------------------------------------------------------------------------------
def test_without_an_axis_exactly_its_sep_cases_flip():
    boxes = [c for c in LINK + SELF if c["kind"] != 1]
    for k in range(15):
        flipped = {c["name"] for c in boxes if rule(c, skip=k) != c["hit"]}
        assert flipped == {c["name"] for c in boxes if c["cls"] == "SEP_%d" % k} and flipped, (k, flipped)


def test_without_a_cylinder_step_exactly_its_cases_flip():
    cyls = [c for c in LINK if c["kind"] == 1]
    steps = [("AXIS", "axis")] + [("EDGE_%d_%d" % (i, c), ("edge", i, c)) for i in range(3) for c in range(4)]
    steps += [("CAP_%d_%d_%d" % (cap, i, sgn), ("cap", cap, i, sgn)) for cap in range(2) for i in range(3) for sgn in range(2)]
    for prefix, skip in steps:
        flipped = {c["name"] for c in cyls if rule(c, skip=skip) != c["hit"]}
        want = {c["name"] for c in cyls if c["cls"] == prefix or (prefix.startswith("CAP") and c["cls"][:-2] == prefix)}
        assert flipped == want and flipped, (prefix, flipped, want)
    # the two caps of a ZEROS_HIT case see the same contact: no single step carries it, the whole cap-plane step does
    for c in cyls:
        if c["cls"] == "ZEROS_HIT":
            A, (Ro, co, (rad, H)) = pair_of(c)
            assert SO.obb_cylinder_overlap(*A, Ro, co, rad, H) and not SI.cylinder_overlap_without_cap_plane(A[0], A[1], A[2], Ro, co, rad, H)


def test_the_exchange_of_the_face_axes_done_by_halves():
    """the cap-plane step with its j / k exchange done by halves (the normal components exchanged, the axes not): every CAP case of an
    exchanged face gets another verdict, no CAP case of a face that is not exchanged does"""
    caps = [c for c in LINK if c["family"] == "CAP"]
    flipped = {c["name"] for c in caps if rule(c, half_swap=True) != c["hit"]}
    assert flipped == {c["name"] for c in caps if c["cls"].endswith("_1")} and len(flipped) >= 12


# ---- the caps of the table -----------------------------------------------------------------------------------------------------------------
def test_caps():
    table = OI.table()
    assert table["margin_m"] == OI.M and len(table["cases"]) == len(LINK) + len(SELF) <= 220
    boxes = [c for c in LINK if c["kind"] == 0]
    for k in range(15):
        for what in ("SEP_%d" % k, "TIGHT_%d" % k):
            assert len({c["link"] for c in boxes if c["cls"] == what}) >= 3, what
    per_link = collections.Counter(c["link"] for c in boxes)
    assert all(per_link[l] >= 3 for l in range(9)), per_link
    caps = [c for c in LINK if c["family"] == "CAP"]
    assert {c["cls"] for c in caps} == {"CAP_%d_%d_%d_%d" % (a, i, s, w) for a in range(2) for i in range(3) for s in range(2) for w in range(2)}
    assert set(range(8)) <= {c["link"] for c in caps}
    edges = {c["cls"] for c in LINK if c["family"] == "EDGE"}
    assert len(edges) >= 10 and edges <= {"EDGE_%d_%d" % (i, c) for i in range(3) for c in range(4)}
    fam = collections.Counter(c["family"] for c in LINK)
    assert fam["AXIS"] >= 3 and fam["CYL_MISS"] >= 3 and fam["ZEROS"] >= 2
    assert {c["cls"] for c in SELF} == {"%s_%d" % (w, k) for w in ("SEP", "TIGHT") for k in range(15)}
    assert len({c["pair"] for c in SELF}) >= 8


# ---- the rows of the GPU test ---------------------------------------------------------------------------------------------------------------
def test_the_shortcut_row_tests_its_midpoint_and_the_midpoint_is_the_case():
    """the three-waypoint row stays inside the limits, its chord's midpoint is q to a few ulps and has q's verdict, and the stage's rule on it
    tests the one candidate (0, 2) and accepts it exactly when the class says miss"""
    for case in LINK:
        x = OI.shortcut_row(case["q"])
        mid = OI.chord_midpoint(x)
        assert OI.in_limits(x[:, 0]) and OI.in_limits(x[:, 1]) and OI.in_limits(x[:, 2]), case["name"]
        assert np.abs(mid - case["q"]).max() <= 4 * np.spacing(np.abs(case["q"]).max()), case["name"]
        assert row_hit(case, mid) == case["hit"], case["name"]
        run = SI.shortcut_row(x, np.asarray(case["oc"])[None], np.array([case["kind"]], dtype=np.int32), 1, K=1)
        assert run["tested"] == 1 and run["accepted"] == (0 if case["hit"] else 1), (case["name"], run["tested"], run["accepted"])


def test_groups_mix_boxes_and_cylinders():
    gs = OI.groups(LINK)
    assert sum(len(g) for g in gs) == len(LINK) and all(1 <= len(g) <= 16 for g in gs)
    assert sum({c["kind"] for c in g} == {0, 1} for g in gs) >= len(gs) - 2, [sorted({c["kind"] for c in g}) for g in gs]
