"""Host side of the self-collision check and of the SDF guide's self-clearance term (no GPU): the pair-mask rule, the input recipe of
the GPU tests and its decision margin, the three entry points in the header, the ctypes table and the library, the guide_cfg keys, and
the refusals that come before anything touches a device."""
import re

import numpy as np
import pytest

from edmp_amd import franka
from tests import self_collision_inputs as I


def test_default_mask_is_the_frame_gap_rule():
    m = franka.self_collision_pairs()
    assert m.shape == (9, 9) and m.dtype == bool
    pairs = [(a, b) for a in range(9) for b in range(9) if m[a, b]]
    want = [(0, b) for b in range(3, 9)] + [(1, b) for b in range(4, 9)] + [(2, b) for b in range(5, 9)] + [(3, b) for b in range(6, 9)]
    assert pairs == want and len(pairs) == 18
    # the rule itself: joint-frame indices at least `min_frame_gap` apart, upper triangle only
    for gap in (0, 1, 2, 3, 6, 7):
        mg = franka.self_collision_pairs(gap)
        for a in range(9):
            for b in range(9):
                assert mg[a, b] == (a < b and franka.LINK_FRAME[b] - franka.LINK_FRAME[a] >= gap), (gap, a, b)
    assert franka.self_collision_pairs(0).sum() == 36 and franka.self_collision_pairs(7).sum() == 0
    assert not franka.self_collision_pairs(1)[6, 7] and not franka.self_collision_pairs(1)[7, 8]  # link7, hand and finger ride one frame
    with pytest.raises(ValueError):
        franka.self_collision_pairs(-1)


def test_check_pair_mask():
    d = franka.check_pair_mask(None)
    assert d.shape == (81,) and d.dtype == np.int32 and d.flags.c_contiguous and np.array_equal(d.reshape(9, 9), franka.self_collision_pairs())
    assert np.array_equal(franka.check_pair_mask(np.zeros((9, 9))), np.zeros(81, dtype=np.int32))
    for bad in (np.zeros((9, 8)), np.zeros(81), np.full((9, 9), 2), np.full((9, 9), 0.5), np.full((9, 9), np.nan)):
        with pytest.raises(ValueError):
            franka.check_pair_mask(bad)


def test_recipe_gives_24_colliding_rows_and_meets_the_condition():
    X, ref = I.rows_and_reference(4)
    assert X.shape == (96, 7, 50) and X.dtype == np.float64
    assert int((~ref["free"]).sum()) == 24 and int(ref["free"].sum()) == 72
    hit = ~ref["free"]
    assert ref["first"][hit].min() == 0 and ref["first"][hit].max() == 47 and (ref["first"][~hit] == -1).all()
    assert (ref["pair"][~hit] == -1).all() and (ref["pair"][hit, 0] < ref["pair"][hit, 1]).all()
    assert all(franka.self_collision_pairs()[a, b] for a, b in ref["pair"][hit])
    print(f"[self-collision inputs] smallest decision distance {ref['decision'].min():.3g} m")
    assert ref["decision"].shape == (96,) and ref["decision"].min() >= I.MIN_DECISION  # (reference() asserts it too: no row is left out)
    assert 1e-6 < ref["decision"].min() < 1e-5  # 7.4e-6 m: the recipe is what the tests were designed on
    # a row on the decision boundary is refused, not dropped
    orig = I.sat_margin
    try:
        I.sat_margin = lambda *a: orig(*a) * 0.0
        with pytest.raises(AssertionError, match="decision boundary"):
            I.reference(X[:2], 4)
    finally:
        I.sat_margin = orig


def test_reference_key_order_on_a_constructed_row():
    """a constant row repeats one configuration: the first colliding configuration is 0 and the pair the first in row-major order"""
    X, ref = I.rows_and_reference(1)  # (substeps 1: every hit sits on a waypoint)
    r = int(np.nonzero(~ref["free"])[0][0])
    w = int(ref["first"][r])
    row = np.repeat(X[r][:, w:w + 1], 5, axis=1)[None]
    one = I.reference(row, 3)
    assert one["first"][0] == 0
    wider = franka.self_collision_pairs().astype(int)
    wider[0, 1] = 1
    every = I.reference(row, 3, wider)
    assert every["first"][0] == 0 and tuple(every["pair"][0]) == (0, 1)  # neighbours overlap by construction
    none = I.reference(row, 3, np.zeros((9, 9), dtype=int))
    assert none["free"][0] and none["first"][0] == -1 and np.isinf(none["decision"][0])


def test_c_abi_declares_the_entry_points():
    from edmp_amd import _capi

    hdr = open(_capi.os.path.join(_capi.os.path.dirname(_capi._HERE), "include", "edmp_hip.h")).read()
    lib = _capi.load()
    for name, nargs in (("edmp_self_collision_rows_dev", 9), ("edmp_sdf_set_self", 6), ("edmp_sdf_self_rows_dev", 9)):
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_capi.SIGNATURES[name][1]) == nargs, name
    # the contract text names the two reports among the calls that leave a segmented run running, not among those that end one
    contract = hdr[hdr.index("A run ends when a segment"):hdr.index("int edmp_denoise_guided_segment_dev")]
    ending, leaving = contract.split("leave a run")
    for name in ("edmp_self_collision_rows_dev", "edmp_sdf_self_rows_dev"):
        assert name in leaving and name not in ending, name


def test_refusals_without_a_device():
    from edmp_amd import _capi
    from edmp_amd.guide import IntersectionVolumeGuide, SceneBatch

    lib = _capi.load()
    mask = franka.check_pair_mask(None)
    assert lib.edmp_self_collision_rows_dev(None, None, 1, 50, 4, None, _capi.as_pi32(mask), None, None) == -1
    assert b"edmp_self_collision_rows_dev" in lib.edmp_last_error()

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError(f"the context was touched ({name}) before the arguments were checked")

    for cls in (IntersectionVolumeGuide, SceneBatch):
        g = object.__new__(cls)
        g.ctx = Untouched()
        for bad in (np.zeros((9, 8)), np.full((9, 9), 3), np.full((9, 9), np.inf)):
            with pytest.raises(ValueError, match="pairs"):
                g.self_collision_rows(np.zeros((1, 7, 50)), pairs=bad)


def test_guide_cfg_keys_of_the_self_term():
    """the cfg dicts of guides 1-13 and 101 are key for key and value for value what they are without the feature; 102 is 101 plus two keys"""
    import yaml

    from edmp_amd import guide_cfg as GC

    T = 255
    base = {"batch_size_per_guide", "total_batch_size", "clearance", "expansion", "guidance_method", "grad_norm", "guidance_schedule", "volume_trust_region"}
    sdf = {"sdf_rows", "sdf_margin", "smoothness"}
    for n in (1, 2, 3, 4, 5, 9, 10, 11, 12, 13):
        assert set(GC.build_guide_cfgs([GC.load_guide_dict(n)], 2, T)) == base, n
        assert "sdf" not in GC.catalog_guide_dict(n)["hyperparameters"]
    c101 = GC.build_guide_cfgs([GC.load_guide_dict(101)], 2, T)
    assert set(c101) == base | sdf and set(GC.catalog_guide_dict(101)["hyperparameters"]["sdf"]) == {"margin", "smoothness"}
    c102 = GC.build_guide_cfgs([GC.load_guide_dict(102)], 2, T)
    assert set(c102) == base | sdf | {"sdf_self_weight", "sdf_self_margin"}
    for k in base | sdf:
        assert np.array_equal(np.asarray(c102[k]), np.asarray(c101[k])), k
    assert c102["sdf_self_weight"].tolist() == [1.0, 1.0] and np.array_equal(c102["sdf_self_margin"], np.tile(np.linspace(0.01, 0.03, T), (2, 1)))
    # a mixed ensemble: zero on the rows of the guides without the term; the YAML round trip carries the keys
    mix = GC.build_guide_cfgs([yaml.safe_load(yaml.safe_dump(GC.catalog_guide_dict(n))) for n in (1, 102, 101)], 2, T)
    assert mix["sdf_self_weight"].tolist() == [0, 0, 1, 1, 0, 0] and not mix["sdf_self_margin"][[0, 1, 4, 5]].any()
    assert "sdf_self_weight" not in GC.build_guide_cfgs([GC.load_guide_dict(n) for n in (1, 101)], 2, T)
    for bad in (dict(self_weight=-1.0), dict(self_weight=float("nan")), dict(self_weight=1.0, self_margin=[0.1, -0.1]), dict(self_weight=1.0, self_margin=[0.1])):
        d = GC.catalog_guide_dict(101)
        d["hyperparameters"]["sdf"].update(bad)
        with pytest.raises(ValueError, match="self_"):
            GC.build_guide_cfgs([d], 2, T)
    d = GC.catalog_guide_dict(1)
    d["hyperparameters"]["sdf"] = dict(self_weight=1.0)
    with pytest.raises(ValueError, match="guidance_method 'sdf'"):
        GC.build_guide_cfgs([d], 2, T)


def test_self_term_tables_are_checked_before_the_library_is_touched():
    from edmp_amd import guide_cfg as GC
    from edmp_amd.guide import sdf_tables

    T = 255
    half = franka.link_half_extents(franka.PLACEHOLDER_LINK_EXTENTS)
    cfgs = GC.build_guide_cfgs([GC.load_guide_dict(n) for n in (1, 102)], 2, T)
    tb = sdf_tables(cfgs, 4, T, half)
    assert tb["self_weight"].tolist() == [0, 0, 1, 1] and tb["self_margin"].shape == (4, T) and tb["self_mask"].shape == (81,)
    assert np.array_equal(tb["self_mask"].reshape(9, 9), franka.self_collision_pairs())
    plain = sdf_tables(GC.build_guide_cfgs([GC.load_guide_dict(101)], 4, T), 4, T, half)
    assert not plain["self_weight"].any() and not plain["self_margin"].any()

    def edited(key, idx, v):
        c = dict(cfgs)
        c[key] = np.array(cfgs[key], dtype=np.float64)
        c[key][idx] = v
        return c

    for what, c in (("weight on an iv row", edited("sdf_self_weight", 0, 1.0)), ("NaN weight", edited("sdf_self_weight", 2, np.nan)),
                    ("negative weight", edited("sdf_self_weight", 2, -1.0)), ("inf margin", edited("sdf_self_margin", (3, 7), np.inf)),
                    ("negative margin", edited("sdf_self_margin", (2, 0), -0.01)), ("shape", dict(cfgs, sdf_self_weight=np.zeros(3)))):
        with pytest.raises(ValueError, match="sdf_self"):
            sdf_tables(c, 4, T, half)
    with pytest.raises(ValueError, match="pairs"):
        sdf_tables(cfgs, 4, T, half, self_pairs=np.full((9, 9), 2))
    # the C entry points refuse a null context by name, without a device
    from edmp_amd import _capi

    lib = _capi.load()
    assert lib.edmp_sdf_set_self(None, None, None, None, 4, T) == -1 and b"edmp_sdf_set_self" in lib.edmp_last_error()
    assert lib.edmp_sdf_self_rows_dev(None, None, 1, 5, 0, 5, 0, None, None) == -1 and b"edmp_sdf_self_rows_dev" in lib.edmp_last_error()
