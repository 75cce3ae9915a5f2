"""Host side of the swept-clearance term of the sphere signed-distance guide: the float64 checker against central differences of its own
cost, the margins of every committed case, the guide_cfg keys (every earlier guide's dict unchanged, value for value), the YAML
validation, the shard slicing and the three C-ABI symbols.  No GPU."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from edmp_amd import guide_cfg as GC
from tests import sdf_reference as R
from tests import sdf_sweep_inputs as I
from tests.util import T

SWEEP_KEYS = ("sdf_sweep_weight", "sdf_sweep_substeps")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guide_cfg_digests_before_sweep.json")


def test_checker_gradient_matches_central_differences():
    """the gradient that evaluate_sweep carries back through the interpolation against (cost(q + h) - cost(q - h)) / 2h on every element
    of two rows with K = 2 and K = 4: <= 1e-6 of the largest element.  h = 1e-6 stays inside the inputs' distance from every kink
    (>= 1e-5 m, and a joint moves a sphere by at most ~1.2 m per rad), so both evaluations see the same active set and the cost is smooth
    between them: truncation ~h^2, rounding ~1e-16 |cost| / h ~ 1e-10 of a gradient of order 1."""
    case = I.check_case("L5_o64_custom_K42")
    rows = list(I.SWEEP_ROWS)
    q = case["joints"][rows]
    rest = case["args"][1:]
    m, w, K = case["cfgs"]["sdf_margin"][rows, I.T_CHECK - 1], case["cfgs"]["sdf_sweep_weight"][rows], case["cfgs"]["sdf_sweep_substeps"][rows]
    assert K.tolist() == [4, 2]
    ref = case["sweept"]["grad"][rows]
    assert np.abs(ref).max() > 0
    h = 1e-6
    num = np.zeros_like(q)
    for idx in np.ndindex(*q.shape):
        r = idx[0]
        qp, qm = q[r:r + 1].copy(), q[r:r + 1].copy()
        qp[(0,) + idx[1:]] += h
        qm[(0,) + idx[1:]] -= h
        cp = I.evaluate_sweep(qp, *rest, m[r:r + 1], w[r:r + 1], int(K[r]), want_grad=False)["cost"][0]
        cm = I.evaluate_sweep(qm, *rest, m[r:r + 1], w[r:r + 1], int(K[r]), want_grad=False)["cost"][0]
        num[idx] = (cp - cm) / (2 * h)
    rel = float(np.abs(num - ref).max() / np.abs(ref).max())
    print(f"[sdf sweep] checker vs central differences: {rel:.3e}")
    assert rel <= 1e-6, rel


def test_interpolants_are_the_success_checks():
    """column w (K - 1) + k - 1 is (1 - k/K) q_w + (k/K) q_{w+1} over start, waypoints, goal; float32 forms them in float32"""
    rs = np.random.RandomState(0)
    q, s, g = rs.uniform(-1, 1, (2, 7, 3)), rs.uniform(-1, 1, 7), rs.uniform(-1, 1, 7)
    Q = I.interpolants(q, s, g, 4)
    assert Q.shape == (2, 7, 12) and Q.dtype == np.float64
    pad = np.concatenate([np.broadcast_to(s.reshape(1, 7, 1), (2, 7, 1)), q, np.broadcast_to(g.reshape(1, 7, 1), (2, 7, 1))], axis=2)
    for w in range(4):
        for k in (1, 2, 3):
            f = k / 4
            assert np.array_equal(Q[:, :, w * 3 + k - 1], (1.0 - f) * pad[:, :, w] + f * pad[:, :, w + 1])
    assert I.interpolants(q, s, g, 4, np.float32).dtype == np.float32
    assert I.interpolants(q, s, g, 2).shape == (2, 7, 4)


@pytest.mark.parametrize("name", list(I.CASES))
def test_margins_of_every_committed_case(name):
    """waypoints and all interpolants >= MIN_GAP from every decision boundary at t = 0 and T_CHECK (check_case asserts it), an active
    hinge among the interpolants and a non-zero sweep gradient on both weighted rows"""
    case = I.check_case(name)
    for mg in (case["margins0"], case["marginst"], case["margins_every"]):
        assert min(mg[k] for k in ("hinge", "obstacle", "axis", "rho")) >= I.MIN_GAP, mg
    assert case["marginst"]["active"] > 0
    assert case["cfgs"]["sdf_sweep_substeps"][list(I.SWEEP_ROWS)].tolist() == list(case["K"])
    print(f"[sdf sweep] {name} seed {case['seed']}: gaps t=0 {case['margins0']}, t={I.T_CHECK} {case['marginst']}, every row {case['margins_every']}")


def test_the_plate_and_the_ends_cases():
    """the plate: +0.077 m at the waypoints, -0.048 m at the segment's midpoint, the waypoint hinge silent (plate_case asserts them); the
    ends: only the start -> q_1 segment is active and only waypoint 1 receives a gradient, by the second-set weights"""
    p = I.plate_case()
    assert p["way0"]["clearance"][0] > 0.07 and p["sweep0"]["clearance"][0] < -0.04 and p["sweep"]["cost"][0] > 0
    e = I.ends_case()
    ev = e["sweep"]["ev"][0]
    gq = ev["grad"][0].reshape(7, 4, 3)  # (joint, segment, k)
    assert gq[:, 0].any() and not gq[:, 1:].any()
    want = (gq[:, 0] * (np.arange(1, 4) / 4)).sum(-1)
    assert np.array_equal(e["sweep"]["grad"][0, :, 0], want)


def digest(cfgs):
    h = hashlib.sha256()
    for k in sorted(cfgs):
        v = np.ascontiguousarray(np.asarray(cfgs[k]))
        h.update(f"{k}|{v.dtype.str}|{v.shape}|".encode())
        h.update(v.tobytes())
    return h.hexdigest()


def test_earlier_guides_keep_their_dicts_value_for_value():
    """guides 1-21 and 101-103: the cfg dict of each (2 rows) has the keys and bytes it had before the term existed - the digests under
    tests/golden were taken from the code without it"""
    want = json.load(open(GOLDEN))
    assert set(want) == {str(n) for n in list(GC.GUIDE_CATALOG) + [101, 102, 103]}
    for n, d in want.items():
        cfgs = GC.build_guide_cfgs([GC.load_guide_dict(int(n))], 2, T)
        assert sorted(cfgs) == d["keys"] and digest(cfgs) == d["sha256"], n
        assert not any(k in cfgs for k in SWEEP_KEYS)


def test_guide_104_is_guide_101_plus_the_two_keys():
    d101, d104 = GC.catalog_guide_dict(101), GC.catalog_guide_dict(104)
    sweep = {k: d104["hyperparameters"]["sdf"].pop(k) for k in ("sweep_weight", "sweep_substeps")}
    d104["index"] = 101
    assert d104 == d101 and sweep == dict(sweep_weight=1.0, sweep_substeps=4)
    c101, c104 = (GC.build_guide_cfgs([GC.load_guide_dict(n)], 2, T) for n in (101, 104))
    assert set(c104) == set(c101) | set(SWEEP_KEYS)
    assert all(np.array_equal(c104[k], c101[k]) for k in c101)
    cfgs = GC.build_guide_cfgs([GC.load_guide_dict(n) for n in (1, 104, 102)], 2, T)
    assert cfgs["sdf_sweep_weight"].tolist() == [0, 0, 1, 1, 0, 0] and cfgs["sdf_sweep_substeps"].tolist() == [4] * 6
    assert cfgs["sdf_sweep_substeps"].dtype == np.int32 and cfgs["sdf_sweep_weight"].dtype == np.float64


def test_bad_sweep_values_raise_with_the_row_named():
    def dicts(**sweep):
        d = [GC.catalog_guide_dict(1), GC.catalog_guide_dict(104), GC.catalog_guide_dict(2)]
        d[1]["hyperparameters"]["sdf"].update(sweep)
        return d

    for sweep, needle in ((dict(sweep_weight=-1.0), "sweep_weight"), (dict(sweep_weight=float("nan")), "sweep_weight"), (dict(sweep_substeps=1), "sweep_substeps"),
                          (dict(sweep_substeps=65), "sweep_substeps"), (dict(sweep_substeps=2.5), "sweep_substeps"), (dict(sweep_weight="1"), "sweep_weight")):
        with pytest.raises(ValueError, match=needle) as e:
            GC.build_guide_cfgs(dicts(**sweep), 3, T)
        assert "guide 104" in str(e.value) and "row 3" in str(e.value), str(e.value)
    d = dicts()
    d[2]["hyperparameters"]["sdf"] = dict(sweep_weight=1.0)  # an iv guide
    with pytest.raises(ValueError, match="guidance_method 'sdf'") as e:
        GC.build_guide_cfgs(d, 3, T)
    assert "guide 2" in str(e.value) and "row 6" in str(e.value)
    # the row arrays themselves, as a guide takes them
    from edmp_amd import franka
    from edmp_amd.guide import sdf_tables

    half = franka.link_half_extents(franka.PLACEHOLDER_LINK_EXTENTS)
    good = GC.build_guide_cfgs(dicts(), 2, T)
    tb = sdf_tables(good, 6, T, half)
    assert tb["sweep_substeps"].dtype == np.int32 and tb["sweep_weight"].tolist() == [0, 0, 1, 1, 0, 0]
    for key, row, val in (("sdf_sweep_weight", 3, -0.5), ("sdf_sweep_substeps", 2, 1), ("sdf_sweep_substeps", 3, 65), ("sdf_sweep_weight", 0, 1.0)):
        bad = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in good.items()}
        bad[key][row] = val
        with pytest.raises(ValueError, match=f"{key}: row {row}"):
            sdf_tables(bad, 6, T, half)
    plain = sdf_tables(GC.build_guide_cfgs([GC.load_guide_dict(101)], 2, T), 2, T, half)  # absent keys: weight 0, substeps 4
    assert not plain["sweep_weight"].any() and plain["sweep_substeps"].tolist() == [4, 4]


def test_shard_guide_cfgs_slices_the_sweep_keys():
    from edmp_amd.dist import shard_guide_cfgs

    cfgs = GC.build_guide_cfgs([GC.load_guide_dict(n) for n in (1, 104, 102)], 4, T)
    sh = shard_guide_cfgs(cfgs, 2, 9)
    for k in SWEEP_KEYS + ("sdf_rows",):
        assert sh[k].shape[0] == 7 and np.array_equal(sh[k], cfgs[k][2:9]), k
    assert not any(k in shard_guide_cfgs(GC.build_guide_cfgs([GC.load_guide_dict(101)], 4, T), 1, 3) for k in SWEEP_KEYS)


def test_c_abi_declares_the_three_entry_points():
    from edmp_amd import _capi

    hdr = open(_capi.os.path.join(_capi.os.path.dirname(_capi._HERE), "include", "edmp_hip.h")).read()
    lib = _capi.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name, nargs in (("edmp_sdf_set_sweep", 4), ("edmp_sdf_sweep_rows_dev", 10), ("edmp_scenes_sdf_sweep_rows_dev", 11)):
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_capi.SIGNATURES[name][1]) == nargs, name
        assert re.search(r"\bT " + name + r"$", exported, re.M), name
    assert re.search(r"#define EDMP_MAX_SWEEP_SUBSTEPS 64\b", hdr) and _capi.MAX_SWEEP_SUBSTEPS == 64
    contract = hdr[hdr.index("A run ends when a segment"):hdr.index("int edmp_denoise_guided_segment_dev")]
    ending, leaving = contract.split("leave a run")
    for name in ("edmp_sdf_sweep_rows_dev", "edmp_scenes_sdf_sweep_rows_dev"):
        assert name in leaving and name not in ending


def test_a_null_context_is_refused_by_name():
    from edmp_amd import _capi

    lib = _capi.load()
    w, k, z = np.ones(2), np.full(2, 4, dtype=np.int32), np.zeros(7)
    assert lib.edmp_sdf_set_sweep(None, _capi.as_pd(w), _capi.as_pi32(k), 2) == -1
    assert (lib.edmp_last_error() or b"").decode().startswith("edmp_sdf_set_sweep")
    assert lib.edmp_sdf_sweep_rows_dev(None, None, 2, 3, 0, _capi.as_pd(z), _capi.as_pd(z), 4, None, None) == -1
    assert (lib.edmp_last_error() or b"").decode().startswith("edmp_sdf_sweep_rows_dev")
    assert lib.edmp_scenes_sdf_sweep_rows_dev(None, None, 1, 2, 5, 0, _capi.as_pd(z), _capi.as_pd(z), 4, None, None) == -1
    assert (lib.edmp_last_error() or b"").decode().startswith("edmp_scenes_sdf_sweep_rows_dev")
    assert C.sizeof(C.c_int) == 4
