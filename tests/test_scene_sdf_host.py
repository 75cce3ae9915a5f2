"""Host side of SDF rows inside a scene batch (no GPU): the concatenation of the scenes' SDF row arrays, the rules SceneBatch applies to
its members before anything is concatenated or bound, and the two entry points in the header, the ctypes table and the library."""
import re

import numpy as np
import pytest

from edmp_amd import franka
from tests import scene_sdf_inputs as I
from tests import sdf_reference as R
from tests.util import T

TODAY = {"n_obstacles", "obstacle_config", "n_classes", "clearance", "expansion", "row_class", "method", "grad_norm", "guidance_schedule"}


def _scene(part, cfgs):
    from edmp_amd.guide import row_classes

    rc, clr, exp = row_classes(np.asarray(cfgs["clearance"]), np.asarray(cfgs["expansion"]))
    out = dict(obstacle_config=part["obstacle_config"], row_class=rc, clearance=clr, expansion=exp, method=np.asarray(cfgs["guidance_method"]),
               grad_norm=np.asarray(cfgs["grad_norm"]), guidance_schedule=np.asarray(cfgs["guidance_schedule"]))
    out.update({k: np.asarray(cfgs[k]) for k in I.SDF_KEYS if k in cfgs})
    return out


def test_scene_batch_tables_concatenate_the_sdf_arrays():
    from edmp_amd.guide import scene_batch_tables

    parts = I.scene_parts()
    tb = scene_batch_tables([_scene(p, p["cfgs"]) for p in parts])
    S, B = I.S, I.B
    assert set(tb) == TODAY | set(I.SDF_KEYS)
    assert tb["sdf_rows"].shape == (S * B,) and tb["sdf_rows"].dtype == np.int32 and tb["sdf_rows"].flags.c_contiguous
    assert tb["sdf_margin"].shape == (S * B, T) and tb["sdf_margin"].dtype == np.float64 and tb["sdf_margin"].flags.c_contiguous
    assert tb["smoothness"].shape == (S * B,) and tb["smoothness"].dtype == np.float64
    for s, p in enumerate(parts):
        rows = slice(s * B, (s + 1) * B)
        for k in I.SDF_KEYS:
            assert np.array_equal(tb[k][rows], np.asarray(p["cfgs"][k])), (s, k)
    # the masks differ from scene to scene, and one scene mixes SDF rows with rows that normalise
    masks = tb["sdf_rows"].reshape(S, B)
    assert len({m.tobytes() for m in masks}) == S and masks.sum(axis=1).tolist() == [4, 6, 6]
    assert (tb["grad_norm"].reshape(S, B)[1] != 0).any() and masks[1].any()
    # some scenes with the arrays and some without, or a wrong shape: refused
    mixed = [_scene(parts[0], p["cfgs"]) if s else _scene(parts[0], I.without_sdf(p["cfgs"])) for s, p in enumerate(parts)]
    with pytest.raises(ValueError, match="scene 0"):
        scene_batch_tables(mixed)
    bad = _scene(parts[1], parts[1]["cfgs"])
    bad["sdf_margin"] = bad["sdf_margin"][:, :-1]
    with pytest.raises(ValueError, match="scene 1"):
        scene_batch_tables([_scene(parts[0], parts[0]["cfgs"]), bad])


def test_scene_batch_tables_without_sdf_keys_are_what_they_were():
    from edmp_amd.guide import scene_batch_tables

    parts = I.scene_parts()
    tb = scene_batch_tables([_scene(p, I.without_sdf(p["cfgs"])) for p in parts])
    assert set(tb) == TODAY
    full = scene_batch_tables([_scene(p, p["cfgs"]) for p in parts])
    for k in TODAY:
        assert tb[k].dtype == full[k].dtype and np.array_equal(tb[k], full[k]), k


def _member(ctx, cfgs, spheres=None):
    """an unbound member as tests/test_sdf_host.py builds it: the host tables SceneBatch's validation reads, nothing else"""
    from edmp_amd.guide import IntersectionVolumeGuide, sdf_tables

    g = object.__new__(IntersectionVolumeGuide)
    g.ctx, g.device, g.batch_size, g.T = ctx, None, 6, T
    g._half, g._dh, g._sf = franka.link_half_extents(), franka.dh_table(), franka.static_frames()
    g._sdf = sdf_tables(cfgs, 6, T, g._half, spheres) if ("sdf_rows" in cfgs or spheres is not None) else None
    return g


def test_scene_batch_validation_of_sdf_members():
    from edmp_amd.guide import SceneBatch

    class Ctx:
        pass

    ctx = Ctx()
    a, b = _member(ctx, R.mixed_cfgs()), _member(ctx, R.mixed_cfgs())
    assert a.has_sdf_rows and b.has_sdf_rows
    # all-SDF passes the validation: the constructor gets as far as the members' tables (these stand-ins have none)
    with pytest.raises(AttributeError, match="obstacle_config"):
        SceneBatch([a, b])
    # different sphere tables
    c = _member(ctx, R.mixed_cfgs(), R.custom_spheres())
    with pytest.raises(ValueError, match="scene 1.*sphere table"):
        SceneBatch([a, c])
    with pytest.raises(ValueError, match="scene 2.*sphere table"):
        SceneBatch([c, _member(ctx, R.mixed_cfgs(), R.custom_spheres()), a])
    # a mix, in either order, names the scene; the member without SDF rows may carry a sphere table of its own
    plain = _member(ctx, R.mixed_cfgs(False), R.custom_spheres())
    assert not plain.has_sdf_rows
    for members, k in (([a, plain], 1), ([plain, plain, a], 2)):
        with pytest.raises(ValueError, match=f"scene {k} has .*SDF rows"):
            SceneBatch(members)


def test_c_abi_declares_the_entry_points():
    from edmp_amd import _capi

    hdr = open(_capi.os.path.join(_capi.os.path.dirname(_capi._HERE), "include", "edmp_hip.h")).read()
    lib = _capi.load()
    for name, nargs in (("edmp_scene_batch_set_sdf", 9), ("edmp_scenes_sdf_rows_dev", 10)):
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_capi.SIGNATURES[name][1]) == nargs, name
    assert "edmp_scenes_sdf_rows_dev" in hdr[hdr.index("A run ends when a segment"):hdr.index("int edmp_denoise_guided_segment_dev")]  # the list of run-ending calls
