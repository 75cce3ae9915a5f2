"""The shortcut stage's rule on the CPU (tests/shortcut_inputs.py): its schedule, its invariants on the GPU tests' cases with the success
check's host twin as the judge, and the admission check that decides which inputs the GPU is compared on exactly."""
import numpy as np
import pytest

from edmp_amd import _capi
from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch
from oracle import success_oracle as SO
from tests import repair_inputs as RI
from tests import shortcut_inputs as I

ENTRY_POINTS = ("edmp_shortcut_rows_dev", "edmp_scenes_shortcut_rows_dev")


def free_rows(X, case, K):
    return SO.success_rows(X, case["obstacle_config"], K, case["kinds"], I.EXTENTS)["first"] < 0


def test_the_library_and_the_objects_carry_the_stage():
    lib = _capi.load()
    for name in ENTRY_POINTS:
        assert name in _capi.SIGNATURES and getattr(lib, name) is not None
    assert callable(IntersectionVolumeGuide.shortcut_rows) and callable(SceneBatch.shortcut_rows)


def test_schedule():
    assert I.schedule(3) == [2]
    assert I.schedule(4) == [3, 2]
    assert I.schedule(50) == [49, 25, 13, 7, 4, 2]
    assert I.schedule(64) == [63, 32, 16, 8, 4, 2]
    for N in range(3, 65):
        s = I.schedule(N)
        assert s[0] == N - 1 and s[-1] == 2 and all(a > b for a, b in zip(s, s[1:])) and s.count(2) == 1


@pytest.mark.parametrize("name", list(I.CASES))
def test_invariants(name):
    """the length never grows, the ends keep their bits, interior waypoints only move inside accepted spans, free stays free by the oracle"""
    case = I.case(name)
    ref, X, K = case["ref"], case["X"], case["K"]
    assert (ref["length"] <= ref["length0"]).all()
    assert np.array_equal(ref["trajectories"][:, :, [0, -1]], X[:, :, [0, -1]])
    before, after = free_rows(X, case, K), free_rows(ref["trajectories"], case, K)
    assert (after | ~before).all()
    for r, run in enumerate(ref["runs"]):
        touched = np.zeros(X.shape[2], dtype=bool)
        for i, j in run["log"]:
            touched[i + 1:j] = True
        assert np.array_equal(ref["trajectories"][r][:, ~touched], X[r][:, ~touched])
        assert run["accepted"] == len(run["log"]) and run["tested"] == len(run["log"]) + len(run["rejected"])
        assert (run["length"] < run["length0"]) == bool(run["log"])


def test_case_conditions():
    """over the cases: at least 20 rejected and 20 accepted candidates, a row whose (0, N - 1) is rejected, a piece of more than 256
    configurations, and every size at which the kernel takes another path: N = 3 (one span), 4, 14, 50, 64; K = 1, 4, 8; 1 and 64 obstacles
    with cylinders; 1 and 5 rows"""
    runs = [(I.case(n), run) for n in I.CASES for run in I.case(n)["ref"]["runs"]]
    assert sum(len(run["rejected"]) for _, run in runs) >= 20 and sum(len(run["log"]) for _, run in runs) >= 20
    assert any((0, c["X"].shape[2] - 1) in run["rejected"] for c, run in runs)
    assert any((j - i) * c["K"] - 1 > 256 for c, run in runs for i, j in run["log"] + run["rejected"])
    assert {c["X"].shape[2] for c, _ in runs} >= {3, 4, 14, 50, 64} and {c["K"] for c, _ in runs} >= {1, 4, 8}
    assert {c["X"].shape[0] for c, _ in runs} >= {1, 5} and {len(c["kinds"]) for c, _ in runs} >= {1, 64}
    assert any(len(c["kinds"]) == 64 and c["kinds"].any() for c, _ in runs)


def test_the_cap_plane_step_alone_decides_candidates():
    """the cylinder test ends with the face x cap-plane segments; shortcut_rows_kernel runs that step in a form of its own (selects, where
    success_rows_kernel indexes).  In the cap-plane cases the rule rejects (0, 2) on every row, and accepts it when that step is left out:
    a fault in the step changes the log that the GPU is compared with.  Both senses of the step's axis swap occur among the cases."""
    names = [n for n in I.CASES if I.CASES[n]["kind"] == "cap_plane"]
    swaps = set()
    for name in names:
        case = I.case(name)
        without = I.shortcut_rows(case["X"], case["obstacle_config"], case["kinds"], case["passes"], case["K"], cap_plane=False)
        for run, alt in zip(case["ref"]["runs"], without["runs"]):
            assert run["log"] == [] and run["rejected"] == [(0, 2)] and alt["log"] == [(0, 2)] and alt["rejected"] == []
        # the face of link box CAP["link"] normal to CAP["axis"] in the cylinder's frame: which in-plane axis has the larger z component
        Ro, _, _, _ = SO.obstacle_shapes(case["obstacle_config"], case["kinds"])
        Rl, _ = SO.link_box_poses((case["X"][0, :, 0] + case["X"][0, :, 2]) / 2)[I.CAP["link"]]
        Rz = (Ro[0].T @ Rl)[2]
        a = I.CAP["axis"]
        swaps.add(bool(abs(Rz[(a + 2) % 3]) > abs(Rz[(a + 1) % 3])))
    assert len(names) >= 4 and swaps == {False, True}


def test_the_stated_rows():
    """the zigzag rows on a graze scene at passes 1 / 2 / 4: accepted, tested and lengths as the stage's description states them"""
    g = RI.graze_scene(0.0)
    want = {14: ((6, 7, 1.380), (12, 14, 1.268), (24, 28, 1.154)), 50: ((28, 29, 1.480), (51, 53, 1.348), (97, 101, 1.261))}
    for N, rows in want.items():
        X = I.zigzag_rows(g["start"], g["goal"], N)
        assert free_rows(X, g, 4).all()
        for passes, (acc, tst, length) in zip((1, 2, 4), rows):
            out = I.shortcut_rows(X, g["obstacle_config"], g["kinds"], passes)
            assert (int(out["accepted"][0]), int(out["tested"][0])) == (acc, tst) and round(float(out["length"][0]), 3) == length
            assert round(float(out["length0"][0]), 3) == {14: 2.851, 50: 9.720}[N] and free_rows(out["trajectories"], g, 4).all()


def test_two_passes_equal_two_runs_of_one():
    for name in ("N14_graze_zigzag", "N4_o7c2_n5"):
        case = I.case(name)
        scene = (case["obstacle_config"], case["kinds"])
        two = I.shortcut_rows(case["X"], *scene, 2, case["K"])
        first = I.shortcut_rows(case["X"], *scene, 1, case["K"])
        second = I.shortcut_rows(first["trajectories"], *scene, 1, case["K"])
        assert np.array_equal(two["trajectories"], second["trajectories"]) and np.array_equal(two["length"], second["length"])
        assert np.array_equal(two["accepted"], first["accepted"] + second["accepted"])
        # (a row whose first pass accepts nothing is not tested again by the one call; the second run tests it once more)
        went_on = first["accepted"] > 0
        assert np.array_equal(two["tested"][went_on], (first["tested"] + second["tested"])[went_on])
        assert np.array_equal(two["tested"][~went_on], first["tested"][~went_on])


def test_a_non_finite_row_is_untouched():
    case = I.case("N4_o7c2_n5")
    for bad in (np.nan, np.inf):
        X = case["X"].copy()
        X[1, 3, 2] = bad
        out = I.shortcut_rows(X, case["obstacle_config"], case["kinds"], 2, case["K"])
        assert out["accepted"][1] == -1 and out["tested"][1] == 0 and np.isnan(out["length0"][1]) and np.isnan(out["length"][1])
        assert np.array_equal(out["trajectories"][1].view(np.int64), X[1].view(np.int64)) and (out["spans"][1] == -1).all()
        keep = [0, 2, 3, 4]
        assert np.array_equal(out["trajectories"][keep], case["ref"]["trajectories"][keep])


def test_admission():
    """the admission check admits the rows the stage's description names and refuses a case put on a decision boundary"""
    for shift in RI.GRAZE_SHIFTS:
        g = RI.graze_scene(shift)
        assert I.admit(g["X"], g["obstacle_config"], g["kinds"], 2)[0]
    p = RI.property_case()
    ok, _, ref = I.admit(p["X"], p["obstacle_config"], p["kinds"], 2)
    assert ok and all(run["log"] == [(0, 13)] for run in ref["runs"])  # (there the straight line is free: every row collapses)
    # a gain on the threshold
    g = RI.graze_scene(0.0)
    X = I.zigzag_rows(g["start"], g["goal"], 14)
    gain = I.shortcut_rows(X, g["obstacle_config"], g["kinds"], 1)["runs"][0]["gains"][0]
    ok, why, _ = I.admit(X, g["obstacle_config"], g["kinds"], 1, min_gain=gain - 1e-10)
    assert not ok and "min_gain" in why
    # an obstacle whose face lies within 1e-6 m of a tested configuration's link box: growing it flips a decision
    case = I.case("N14_graze_zigzag")
    Q = I.piece_configurations(I.piece(case["X"][0], 0, 13), case["K"])  # (alone with that cube, the whole chord is the first candidate)
    oc = touching_cube(Q, case["kinds"][:1])
    ok, why, _ = I.admit(case["X"], oc, case["kinds"][:1], 1, case["K"])
    assert not ok and "another log" in why


def touching_cube(Q, kinds):
    """one axis-aligned 0.1 m cube placed above the highest link-box corner of the configurations Q, its lower face 2.5e-7 m away from it"""
    from edmp_amd import franka

    he = franka.link_half_extents(I.EXTENTS).astype(np.float64)
    Rl, cl = SO.link_box_poses_batch(Q)
    top = (cl[:, :, 2] + np.einsum("mlk,lk->ml", np.abs(Rl[:, :, 2, :]), he))
    m, l = np.unravel_index(np.argmax(top), top.shape)
    corner = cl[m, l] + Rl[m, l] @ (np.sign(Rl[m, l][2, :]) * he[l])
    oc = np.array([[corner[0], corner[1], top[m, l] + 2.5e-7 + 0.05, 0.0, 0.0, 0.0, 1.0, 0.1, 0.1, 0.1]])
    assert not I.any_hit(Q, oc, kinds) and I.any_hit(Q, I.grown(oc, I.GROW), kinds)
    return oc
