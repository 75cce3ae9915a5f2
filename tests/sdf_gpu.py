"""What the GPU tests of the sphere signed-distance guide and its terms share (test_gpu_sdf, test_gpu_sdf_self, test_gpu_sdf_goal,
test_gpu_sdf_sweep, test_gpu_sdf_terms, test_gpu_scene_sdf, test_gpu_repair): building a guide from a case or one per scene, the tiny net
and the ensembles of the runs, the gradient with its sum of squares, and the parity records."""
import json
import os

import numpy as np
import pytest
import torch

DEV = "cuda:0"


def build_guide(case, cfgs=None, **kw):
    """the guide of a checker case: its obstacles and kinds, the placeholder link boxes, its sphere table where the case says "custom",
    its tool frame where it has one; cfgs replaces the case's own"""
    from edmp_amd import franka
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = case["cfgs"] if cfgs is None else cfgs
    kw.setdefault("obstacle_kinds", case["kinds"])
    if "tool" in case:
        kw.setdefault("goal_tool", case["tool"])
    return IntersectionVolumeGuide(case["obstacle_config"], DEV, cfgs, cfgs["total_batch_size"], link_mesh_extents=franka.PLACEHOLDER_LINK_EXTENTS,
                                   spheres=case["spheres"] if case.get("custom") else None, **kw)


def scene_guides(parts, device=DEV, cfgs=None, each=lambda s: {}, **kw):
    """one guide per scene of scene_sdf_inputs.scene_parts, with the scene's own cfgs unless cfgs lists others; each(s): scene s's own keywords"""
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = [p["cfgs"] for p in parts] if cfgs is None else cfgs
    return [IntersectionVolumeGuide(p["obstacle_config"], device, cfgs[s], cfgs[s]["total_batch_size"], obstacle_kinds=p["kinds"], **each(s), **kw)
            for s, p in enumerate(parts)]


def tiny_unet(device=DEV, max_batch=64):
    from edmp_amd import weights as W
    from edmp_amd.temporalunet import TemporalUNet
    from tests.util import TINY_DIMS

    return TemporalUNet(None, 7, 32, device, dims=TINY_DIMS, state_dict=W.init_state_dict(5, 7, 32, TINY_DIMS), max_batch=max_batch)


@pytest.fixture(scope="module")
def tiny_net():
    """a test module imports this fixture and so builds its own net, once"""
    return tiny_unet()


def with_guide(guides, n):
    """a guide list with sample guide n in the place of guide 101"""
    return [n if g == 101 else g for g in guides]


def run_cfgs(n):
    """four rows each of guide 1, the SDF guide n and guide 13, whose rows normalise"""
    from edmp_amd import guide_cfg as GC
    from tests.sdf_reference import T

    return GC.build_guide_cfgs([GC.load_guide_dict(g) for g in (1, n, 13)], 4, T)


def gradient_and_sumsq(guide, joints, start, goal, t):
    """get_gradient with the whole batch's sum g^2 (before mixing) read back as well"""
    from edmp_amd import _capi
    from edmp_amd.runtime import ptr

    guide._bind()
    ctx = guide.ctx
    ji = ctx.to_dev(np.asarray(joints, dtype=np.float64), torch.float64)
    n, L = ji.shape[0], ji.shape[2]
    out, sq = ctx.empty((n, 7, L), torch.float64), ctx.empty((1,), torch.float64)
    s, g = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(7)) for v in (start, goal))
    _capi.check(ctx.lib.edmp_guide_gradient_dev(ctx.h, ptr(ji), n, L, _capi.as_pd(s), _capi.as_pd(g), int(t), ptr(out), ptr(sq)), "edmp_guide_gradient_dev")
    return ctx.to_host(out), float(ctx.to_host(sq)[0])


def recorder(tag, env, gate):
    """(record, fixture) of a test module: record(**kw) prints a comparison as "[tag] {json}" and keeps it; the module-scoped autouse
    fixture writes {"gate": gate, "records": [...]} to the file that the environment variable `env` names, if it names one"""
    records = []

    def record(**kw):
        records.append(kw)
        print(f"[{tag}]", json.dumps(kw))

    @pytest.fixture(scope="module", autouse=True)
    def _write_records():
        yield
        out = os.environ.get(env)
        if out:
            with open(out, "w") as f:
                json.dump({"gate": gate, "records": records}, f, indent=1)

    return record, _write_records
