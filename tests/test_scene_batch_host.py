"""Host side of scene batches (no GPU): the concatenation of S scenes' tables and rows, the placement of every scene's noise in the
batch layout, and the argument checks of Diffusion.denoise_guided_scenes, which must reject bad input before touching the GPU."""
import numpy as np
import pytest
import torch

from tests.util import T, cfgs_for


def _scene(no, guides, bpg, seed):
    from edmp_amd.guide import row_classes
    from edmp_amd.scenes import random_scene

    cfgs = cfgs_for(guides, bpg)
    rc, clr, exp = row_classes(np.asarray(cfgs["clearance"]), np.asarray(cfgs["expansion"]))
    return dict(obstacle_config=random_scene(seed, no), row_class=rc, clearance=clr, expansion=exp, method=np.asarray(cfgs["guidance_method"]),
                grad_norm=np.asarray(cfgs["grad_norm"]), guidance_schedule=np.asarray(cfgs["guidance_schedule"])), cfgs


def test_scene_batch_tables_renumber_classes_per_scene():
    from edmp_amd.guide import scene_batch_tables

    parts = [_scene(4, [1, 5, 10], 8, 1), _scene(16, [11, 13], 12, 2), _scene(64, [13, 1, 11, 5], 6, 3)]
    sc = [p[0] for p in parts]
    tb = scene_batch_tables(sc)
    B = 24
    assert tb["n_obstacles"].tolist() == [4, 16, 64]
    assert tb["n_classes"].tolist() == [s["clearance"].shape[0] for s in sc]
    assert np.array_equal(tb["obstacle_config"], np.concatenate([s["obstacle_config"] for s in sc]))
    off = np.concatenate([[0], np.cumsum(tb["n_classes"])])
    for s, (scene, cfgs) in enumerate(parts):
        rows = slice(s * B, (s + 1) * B)
        cls = tb["row_class"][rows]
        # every row of scene s indexes one of scene s's classes, and that class holds the row's own schedules
        assert np.all((cls >= off[s]) & (cls < off[s + 1]))
        assert np.array_equal(tb["clearance"][cls], np.asarray(cfgs["clearance"]))
        assert np.array_equal(tb["expansion"][cls], np.asarray(cfgs["expansion"]))
        assert np.array_equal(tb["method"][rows], np.asarray(cfgs["guidance_method"], dtype=np.float32))
        assert np.array_equal(tb["grad_norm"][rows], np.asarray(cfgs["grad_norm"]))
        assert np.array_equal(tb["guidance_schedule"][rows], np.asarray(cfgs["guidance_schedule"]))
    assert tb["row_class"].dtype == np.int32 and tb["row_class"].shape == (3 * B,)


def test_scene_batch_tables_refuse_bad_scenes():
    from edmp_amd.guide import scene_batch_tables

    a, _ = _scene(4, [1, 5], 12, 1)
    b, _ = _scene(4, [1], 12, 2)  # 12 rows against 24
    with pytest.raises(ValueError, match="same rows"):
        scene_batch_tables([a, b])
    with pytest.raises(ValueError, match="1..16 scenes"):
        scene_batch_tables([a] * 17)
    with pytest.raises(ValueError, match="1..16 scenes"):
        scene_batch_tables([])
    c = dict(a, obstacle_config=np.zeros((65, 10)))
    with pytest.raises(ValueError, match="obstacles"):
        scene_batch_tables([a, c])


def test_noise_chunk_places_every_scene_at_its_rows():
    from edmp_amd.diffusion import place_scene_rows

    S, B, steps = 3, 5, 4
    pieces = [torch.arange(steps * B * 7 * 2, dtype=torch.float64).view(steps, B, 7, 2) + 1000 * s for s in range(S)]
    dst = torch.full((steps, S * B, 7, 2), float("nan"), dtype=torch.float64)
    place_scene_rows(dst, pieces)
    for k in range(steps):
        for s in range(S):
            assert torch.equal(dst[k, s * B:(s + 1) * B], pieces[s][k])
    with pytest.raises(ValueError):
        place_scene_rows(torch.empty((steps, S * B + 1, 7, 2), dtype=torch.float64), pieces)
    with pytest.raises(ValueError):
        place_scene_rows(dst, [pieces[0][:2]] * S)


class _NoGpu:
    """a context stand-in: any use of it means the call went past its argument checks"""

    def __getattr__(self, name):
        raise AssertionError(f"argument checks let the call reach the context ({name})")


def _fakes(S=3, B=4, max_batch=12):
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import SceneBatch

    ctx = _NoGpu()
    dif = object.__new__(Diffusion)
    dif.__dict__.update(ctx=ctx, T=T, variance_thresh=0.02)
    batch = object.__new__(SceneBatch)
    batch.__dict__.update(ctx=ctx, n_scenes=S, batch_size=B)

    class Model:
        pass

    m = Model()
    m.__dict__.update(ctx=ctx, horizon=50, input_dim=7, max_batch=max_batch)
    return dif, batch, m


@pytest.mark.parametrize("case", ["not_a_batch", "traj_len", "max_batch", "t_stop", "starts_shape", "goals_missing", "noise_len", "noise_shape",
                                  "device_noise", "noise_mixed"])
def test_denoise_guided_scenes_checks_arguments_first(case):
    from edmp_amd import _capi

    dif, batch, model = _fakes()
    S, B = 3, 4
    st, gl = np.zeros((S, 7)), np.zeros((S, 7))
    kw = dict(noise=[np.zeros((T + 1, B, 7, 50))] * S)
    args = [model, batch, 50, 7, st, gl]
    err = ValueError
    if case == "not_a_batch":
        args[1] = object()
    elif case == "traj_len":
        args[2] = 48
    elif case == "max_batch":
        model.max_batch = S * B - 1
    elif case == "t_stop":
        kw["t_stop"] = T
    elif case == "starts_shape":
        args[4] = np.zeros((S - 1, 7))
    elif case == "goals_missing":
        args[5] = None
    elif case == "noise_len":
        kw["noise"] = kw["noise"][:2]
    elif case == "noise_shape":
        kw["noise"] = [np.zeros((T + 1, B + 1, 7, 50))] * S
    elif case == "device_noise":
        kw["noise"], err = "device", _capi.EdmpError
    elif case == "noise_mixed":
        kw["noise"] = [torch.zeros((T + 1, B, 7, 50), dtype=torch.float64).pin_memory() if torch.cuda.is_available() else torch.zeros(1)] + kw["noise"][1:]
    with pytest.raises(err):
        dif.denoise_guided_scenes(*args, **kw)
