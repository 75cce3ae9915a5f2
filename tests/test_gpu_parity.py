"""GPU parity tests: the HIP path (through the C-ABI of libedmp_hip.so) against the CPU oracle and against the
golden vectors captured from the unmodified reference.  Tolerances follow BASELINE.json's north star: joint-angle
RMSE <= 1e-4 per step (teacher-forced); individual kernels are held to much tighter bounds."""
import os

import numpy as np
import pytest
import torch
from ctypes import byref, c_int as C_int

from tests.util import FULL_DIMS, T, TINY_DIMS, cfgs_for, maxabs, noise_for, rmse

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def oracle():
    from oracle import edmp_oracle as O

    return O


@pytest.fixture(scope="module")
def tiny_net():
    from edmp_amd import weights as W
    from edmp_amd.temporalunet import TemporalUNet

    sd = W.init_state_dict(5, 7, 32, TINY_DIMS)
    return TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=sd, max_batch=64), sd


def test_native_library_loaded():
    from edmp_amd import _capi

    lib = _capi.load()
    assert lib.edmp_version() >= 100
    with open("/proc/self/maps") as f:
        assert "libedmp_hip.so" in f.read()


def test_schedule(golden):
    from edmp_amd.diffusion import Diffusion

    d = Diffusion(T, DEV)
    g = golden("g2_schedule")
    for k in ("beta", "alpha", "alpha_bar"):
        assert np.array_equal(getattr(d, k), g[k]), k  # f64 tables are bit-exact


def test_psample(golden):
    from edmp_amd.diffusion import Diffusion

    d = Diffusion(T, DEV)
    g = golden("g7_psample")
    for t in (255, 128, 2, 1):
        np.random.seed(int(g["seed_base"]) + t)
        out = d.p_sample_using_posterior(g["x"], t, g["eps"])
        assert maxabs(out, g[f"x_out_t{t}"]) <= 1e-14, t
    # Q3: at t == 1 only row 0 of z is dropped
    np.random.seed(1)
    z = np.random.standard_normal(g["x"].shape)
    a = d.p_sample_using_posterior(g["x"], 1, g["eps"], z=z)
    z0 = z.copy()
    z0[0] = 0
    b = d.p_sample_using_posterior(g["x"], 2, g["eps"], z=z0)  # different t: only checks z handling below
    assert not np.allclose(a[1], d.p_sample_using_posterior(g["x"], 1, g["eps"], z=np.zeros_like(z))[1])


@pytest.mark.parametrize("tag,dims", [("tiny", TINY_DIMS), ("full", FULL_DIMS)])
def test_unet_golden(golden, tag, dims):
    from edmp_amd import weights as W
    from edmp_amd.temporalunet import TemporalUNet

    g = golden(f"g8_unet_{tag}")
    sd = W.init_state_dict(int(g["seed"]), 7, 32, dims)
    net = TemporalUNet(None, 7, 32, DEV, dims=dims, state_dict=sd, max_batch=8)
    x = torch.from_numpy(g["x"])
    for tt in (255, 37, 1):
        eps = net(x, torch.tensor([float(tt)])).cpu().numpy()
        ref = g[f"eps_t{tt}"]
        assert rmse(eps, ref) <= 2e-5 and maxabs(eps, ref) <= 2e-4, (tt, rmse(eps, ref), maxabs(eps, ref))
        if tt == 37:  # intermediate activations localise a failure
            n_lv = len(dims)
            from edmp_amd import _capi

            for i in range(n_lv):
                try:
                    a = net.activation(i, x.shape[0]).cpu().numpy()
                except _capi.EdmpError:
                    # the first two down levels of the full-size net are one launch (level.hip: level2_kernel, round 5): level 0's
                    # output only ever exists in LDS; the tap of level 1 right behind it covers it
                    assert i == 0 and tag == "full"
                    continue
                assert maxabs(a, g[f"trace_down{i}"]) <= 5e-4, f"down{i}"
            assert maxabs(net.activation(100, x.shape[0]).cpu().numpy(), g["trace_mid"]) <= 5e-4

            for j in range(n_lv - 1):
                try:
                    a = net.activation(200 + j, x.shape[0]).cpu().numpy()
                except _capi.EdmpError:
                    # the last up level of the full-size net is one launch together with final_conv.0 (level.hip): its
                    # up-sampled activation never exists in HBM; eps above covers it
                    # (and, when EDMP_LEVEL_MERGE bit 1 is on, the level before it is part of the same launch)
                    assert j >= n_lv - 3 and tag == "full"
                    continue
                assert maxabs(a, g[f"trace_up{j}"]) <= 5e-4, f"up{j}"


def test_unet_vs_oracle_ragged_batches(oracle, tiny_net):
    net, sd = tiny_net
    ou = oracle.UNetOracle(sd)
    rs = np.random.RandomState(0)
    for B in (1, 3, 33, 64):  # not multiples of the 64/128-sample tiles
        x = torch.tensor(rs.standard_normal((B, 7, 50)) * 2, dtype=torch.float32)
        for tt in (1.0, 200.0):
            a = net(x, torch.tensor([tt])).cpu().numpy()
            b = ou(x, torch.tensor([tt])).numpy()
            assert rmse(a, b) <= 2e-5, (B, tt, rmse(a, b))


def test_full_unet_fused_kernels_vs_oracle_ragged(oracle, monkeypatch):
    """Full-size net (the fused conv+GroupNorm kernels only exist for its channel widths), batch sizes that are
    not multiples of any tile (32-sample / 2,4,5,9-sample workgroups), every level's activation checked."""
    from edmp_amd import weights as W
    from edmp_amd.temporalunet import TemporalUNet

    sd = W.init_state_dict(11, 7, 32, FULL_DIMS)
    net = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=80)
    # level 0's output has no HBM tap in the default program (the first two down levels are one launch, round 5): a second model
    # built with one launch per level serves that tap
    monkeypatch.setenv("EDMP_LEVEL_MERGE", "0")
    net_split = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=80)
    monkeypatch.delenv("EDMP_LEVEL_MERGE")
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    rs = np.random.RandomState(2)
    for B in (1, 37, 67):
        x = torch.tensor(rs.standard_normal((B, 7, 50)) * 1.5, dtype=torch.float32)
        tr = {}
        with torch.no_grad():
            ref = oracle.unet_forward(tsd, x, torch.tensor([123.0]), trace=tr).numpy()
        eps = net(x, torch.tensor([123.0])).cpu().numpy()
        assert rmse(eps, ref) <= 2e-5 and maxabs(eps, ref) <= 2e-4, (B, rmse(eps, ref), maxabs(eps, ref))
        eps_split = net_split(x, torch.tensor([123.0])).cpu().numpy()
        assert rmse(eps_split, ref) <= 2e-5 and maxabs(eps_split, ref) <= 2e-4, (B, "one launch per level")
        assert maxabs(net_split.activation(0, B).cpu().numpy(), tr["down0"].numpy()) <= 5e-4, (B, "down0")
        net(x, torch.tensor([123.0]))  # (re-bind the default model: taps read the activations of the last forward)
        for i in range(1, 6):
            assert maxabs(net.activation(i, B).cpu().numpy(), tr[f"down{i}"].numpy()) <= 5e-4, (B, f"down{i}")
        assert maxabs(net.activation(100, B).cpu().numpy(), tr["mid"].numpy()) <= 5e-4
        for j in range(4):  # up4's activation stays on chip: that level runs as one launch with final_conv.0 (level.hip); eps covers it
            from edmp_amd import _capi

            try:
                a = net.activation(200 + j, B).cpu().numpy()
            except _capi.EdmpError:  # (a level merged with its successor has no tap: the one-launch-per-level model serves it)
                a = net_split.activation(200 + j, B).cpu().numpy()
            assert maxabs(a, tr[f"up{j}"].numpy()) <= 5e-4, (B, f"up{j}")


def test_fused_and_unfused_paths_agree(monkeypatch):
    """EDMP_NO_FUSED=1 builds the same network from the generic conv + separate GroupNorm kernels."""
    from edmp_amd import weights as W
    from edmp_amd.temporalunet import TemporalUNet

    sd = W.init_state_dict(12, 7, 32, FULL_DIMS)
    x = torch.tensor(np.random.RandomState(4).standard_normal((33, 7, 50)), dtype=torch.float32)
    a = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=33)(x, torch.tensor([9.0])).cpu().numpy()
    # every program-builder switch gives the same network: no residual fold, no whole-level kernels (the 32/64-channel
    # levels on the generic conv + GroupNorm kernels), no fusion at all (the generic fallback everywhere)
    for env in ("EDMP_NO_RESFOLD", "EDMP_NO_LEVEL", "EDMP_NO_FUSED"):
        monkeypatch.setenv(env, "1")
        b = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=33)(x, torch.tensor([9.0])).cpu().numpy()
        monkeypatch.delenv(env)
        assert rmse(a, b) <= 1e-5, (env, rmse(a, b))


def test_sixteen_sample_tiles_of_the_direct_form_instances(monkeypatch):
    """Round 5: the direct-form position-tile instances of the 256 / 512-channel levels (Conv1dBlock at L = 7, the k3s2 / ConvTranspose
    resamplers) exist with 16-sample tiles (v_mfma_f32_16x16x4_f32, two workgroups per CU) beside the 32-sample ones; EDMP_MS16=<mask>
    picks per family at model-build time (unet.hip: choose_conv).  Same arithmetic, another summation order: every mask gives the network
    of the oracle within the gates of test_unet_golden, whole and ragged batches, and the families all differ from mask 0 only by rounding."""
    from edmp_amd import weights as W
    from edmp_amd.temporalunet import TemporalUNet
    from oracle import edmp_oracle as O

    sd = W.init_state_dict(12, 7, 32, FULL_DIMS)
    x = torch.tensor(np.random.RandomState(4).standard_normal((70, 7, 50)), dtype=torch.float32)
    t = torch.tensor([9.0])
    ref = O.UNetOracle(sd)(x, t).numpy()
    outs = {}
    monkeypatch.setenv("EDMP_BF16X3", "0")  # the fp32-MFMA instances are the subject here (round 6 runs these layers on bf3.hip by default)
    for mask in ("0x00", "0x01", "0x04", "0x1f"):
        monkeypatch.setenv("EDMP_MS16", mask)
        net = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=70)
        monkeypatch.delenv("EDMP_MS16")
        y = net(x, t).cpu().numpy()
        names = {n for n, _, _, _ in net.ctx.prof_ops()}  # the bound model's layer program
        y33 = net(x[:33], t).cpu().numpy()
        assert np.array_equal(y33, y[:33]), mask  # rows are independent of the batch they sit in
        assert rmse(y, ref) <= 2e-5 and maxabs(y, ref) <= 2e-4, (mask, rmse(y, ref), maxabs(y, ref))
        outs[mask] = (y, names)
    for mask in ("0x01", "0x04", "0x1f"):
        assert rmse(outs[mask][0], outs["0x00"][0]) <= 1e-5, mask
    n0, n31 = outs["0x00"][1], outs["0x1f"][1]
    if n0 and n31:  # the layer program really switched instances
        assert "wide_conv_kernel<0, 32, 32, 32, 7, false>" in n0 and "wide_conv_kernel<0, 16, 32, 32, 7, false>" in n31
        assert "wide_conv_kernel<2, 16, 64, 64, 2, false>" in n31 and "wide_conv_kernel<1, 16, 64, 64, 4, false>" in n31


@pytest.mark.parametrize("mask", ["1", "2", "3"])
def test_merged_levels_are_bit_identical_to_two_launches(monkeypatch, mask):
    """Round 5: EDMP_LEVEL_MERGE bit 0 runs the two down levels of the 32 / 64-channel resolutions as ONE launch (level.hip:
    level2_kernel), level 1's k3s2 output handed to level 2 in LDS; bit 1 does the same for the two last up levels (the ConvTranspose
    output of the 64-channel level = the first half of the last level's input tile).  Both levels execute level_body's code on two
    samples per workgroup, so the forward equals the one-launch-per-level program built with two samples per workgroup
    (EDMP_LEVEL_SB=2222) BIT FOR BIT - whole, ragged and tiny batches, also through the fused step tail of the device-resident loop -
    and the oracle within the usual gates; the handed-over activation has no HBM tap any more."""
    from edmp_amd import _capi
    from edmp_amd import weights as W
    from edmp_amd.temporalunet import TemporalUNet
    from oracle import edmp_oracle as O

    sd = W.init_state_dict(12, 7, 32, FULL_DIMS)
    x = torch.tensor(np.random.RandomState(4).standard_normal((70, 7, 50)), dtype=torch.float32)
    t = torch.tensor([9.0])
    monkeypatch.setenv("EDMP_LEVEL_SB", "2222")
    monkeypatch.setenv("EDMP_LEVEL_MERGE", "0")
    two = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=70)
    monkeypatch.setenv("EDMP_LEVEL_MERGE", mask)
    one = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=70)
    monkeypatch.delenv("EDMP_LEVEL_MERGE")
    monkeypatch.delenv("EDMP_LEVEL_SB")
    m = int(mask)
    for B in (70, 33, 5, 1):
        a, b = two(x[:B], t).cpu().numpy(), one(x[:B], t).cpu().numpy()
        assert np.array_equal(a, b), B
        if B == 70:
            for tap in (1, 202):
                assert np.array_equal(two.activation(tap, B).cpu().numpy(), one.activation(tap, B).cpu().numpy()), tap
            names = {n for n, _, _, _ in one.ctx.prof_ops()}
            assert ("level2_kernel<0, 32, 50, 8, 0, 64, 25, 32, 2>" in names) == bool(m & 1)
            assert ("level2_kernel<1, 64, 13, 256, 2, 32, 25, 128, 2>" in names) == bool(m & 2)
            for bit, tap in ((1, 0), (2, 203)):
                if m & bit:
                    with pytest.raises(_capi.EdmpError):
                        one.activation(tap, B)
                else:
                    assert np.array_equal(two.activation(tap, B).cpu().numpy(), one.activation(tap, B).cpu().numpy()), tap
    ref = O.UNetOracle(sd)(x, t).numpy()
    y = one(x, t).cpu().numpy()
    assert rmse(y, ref) <= 2e-5 and maxabs(y, ref) <= 2e-4
    # the device-resident loop: the step tail runs inside the last level's launch - also when that launch is the merged pair
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion

    dif = Diffusion(T, DEV)
    noise = dif.ctx.to_dev(np.random.RandomState(4).standard_normal((T + 1, 70, 7, 50)), torch.float64)
    kw = dict(batch_size=70, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL, noise=noise, t_stop=T - 6)
    assert np.array_equal(dif.denoise_guided(two, None, 50, 7, None, **kw), dif.denoise_guided(one, None, 50, 7, None, **kw))


def test_obstacle_table(golden):
    from edmp_amd.guide import IntersectionVolumeGuide

    g = golden("g3_obstacles")
    cfgs = cfgs_for(g["guides"], g["bpg"])
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, cfgs["total_batch_size"])
    for i, t in enumerate(g["ts"]):
        guide.define_obstacles(None, int(t))
        assert maxabs(guide.obs_min.numpy(), g["obs_min"][i]) <= 2e-7, t
        assert maxabs(guide.obs_max.numpy(), g["obs_max"][i]) <= 2e-7, t


def test_costs_golden(golden):
    from edmp_amd.guide import IntersectionVolumeGuide

    g = golden("g5_costs")
    cfgs = cfgs_for(g["guides"], g["bpg"])
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, cfgs["total_batch_size"])
    q = torch.tensor(g["joints"], dtype=torch.float32)
    for t in (0, 6, 128, 254):
        iv = guide.cost(q, t).cpu().numpy()
        sv = guide.swept_volume_cost(q, torch.tensor(g["start"], dtype=torch.float32), torch.tensor(g["goal"], dtype=torch.float32), t).cpu().numpy()
        assert iv.shape == g[f"iv_t{t}"].shape and sv.shape == g[f"sv_t{t}"].shape
        assert maxabs(iv, g[f"iv_t{t}"]) <= 2e-7, t   # volumes are O(1e-2): ~1e-5 relative
        assert maxabs(sv, g[f"sv_t{t}"]) <= 2e-7, t


def test_ik_filter_cost(golden):
    from edmp_amd.guide import IntersectionVolumeGuide

    g = golden("g11_ik_filter")
    cfgs = cfgs_for([1, 10, 11, 18, 9, 13], 2)
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, 12)
    ik = g["ik"]
    vols = guide.cost(torch.tensor(ik.reshape((-1, 7, 1))), 0, batch_size=ik.shape[0]).sum(axis=(1, 2)).cpu().numpy()
    assert maxabs(vols, g["volumes"]) <= 1e-6
    assert int(np.argmin(vols)) == int(np.argmin(g["volumes"]))


def test_gradient_golden(golden):
    from edmp_amd.guide import IntersectionVolumeGuide

    g = golden("g6_gradient")
    cfgs = cfgs_for(g["guides"], g["bpg"])
    B = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, B)
    for t in (6, 128, 254):
        out = guide.get_gradient(g["joints"], g["start"], g["goal"], t)
        ref = g[f"grad_t{t}"]
        assert out.dtype == np.float64 and out.shape == ref.shape
        # gradient entries reach ~10; autograd itself is only f32-accurate
        assert maxabs(out, ref) <= 2e-5 and rmse(out, ref) <= 2e-6, (t, maxabs(out, ref), rmse(out, ref))
    out = guide.get_gradient(g["joints_ties"], g["start"], g["goal"], 128)
    assert maxabs(out, g["grad_ties_t128"]) <= 2e-5, "tie conventions (identical consecutive waypoints)"
    # Q7: all-zero gradient -> NaN everywhere, also for rows without grad_norm
    far = IntersectionVolumeGuide(g["scene_far"], DEV, cfgs, B)
    assert np.isnan(far.get_gradient(g["joints"], g["start"], g["goal"], 128)).all()
    cfg6 = cfgs_for([1, 2, 3, 4, 5, 10], 2)
    far6 = IntersectionVolumeGuide(g["scene_far"], DEV, cfg6, 12)
    assert np.isnan(far6.get_gradient(g["joints"], g["start"], g["goal"], 128)).all()


def test_guide_built_from_a_mesh_directory(golden, oracle, tmp_path):
    """a8: a guide whose link boxes were measured from .obj meshes (G15, the reference's reader) = a guide handed the same table,
    and both follow the oracle built with that table (not the placeholder's boxes)."""
    from edmp_amd import franka, scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    g = golden("g15_link_meshes")
    for name, text in zip(g["link_names"], g["obj_texts"]):
        with open(os.path.join(str(tmp_path), str(name) + ".obj"), "w") as f:
            f.write(str(text))
    cfgs = cfgs_for([1, 10, 11], 2)
    B = cfgs["total_batch_size"]
    scene = scenes.random_scene(3, 8)
    ga = IntersectionVolumeGuide(scene, DEV, cfgs, B, mesh_dir=str(tmp_path))
    assert np.array_equal(ga.link_dimensions.numpy(), g["link_dimensions"])
    gb = IntersectionVolumeGuide(scene, DEV, cfgs, B, link_mesh_extents=franka.link_extents_from_mesh_dir(tmp_path))
    gp = IntersectionVolumeGuide(scene, DEV, cfgs, B, link_mesh_extents=franka.PLACEHOLDER_LINK_EXTENTS)
    og = oracle.GuideOracle(scene, cfgs, B, link_mesh_extents=ga.link_mesh_extents)
    rs = np.random.RandomState(5)
    lo, hi = oracle.joint_limits()
    q = rs.uniform(lo[None, :, None], hi[None, :, None], (B, 7, 48))
    s, gl = scenes.random_start_goal(9)
    a, b, c = (x.get_gradient(q, s, gl, 100) for x in (ga, gb, gp))
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    o = og.get_gradient(q, s, gl, 100)
    assert maxabs(a, o) <= 5e-5 and rmse(a, o) <= 3e-6, (maxabs(a, o), rmse(a, o))


def test_gradient_vs_oracle_random(oracle):
    """seeded random inputs, many obstacles, every shipped guide class."""
    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    guides = sorted(GC.GUIDE_CATALOG)
    cfgs = cfgs_for(guides, 3)
    B = cfgs["total_batch_size"]
    scene = scenes.random_scene(3, 32)
    guide = IntersectionVolumeGuide(scene, DEV, cfgs, B)
    og = oracle.GuideOracle(scene, cfgs, B)
    rs = np.random.RandomState(5)
    lo, hi = oracle.joint_limits()
    q = oracle.clip_joints(rs.uniform(lo[None, :, None] - 0.3, hi[None, :, None] + 0.3, (B, 7, 48)))
    s, gl = scenes.random_start_goal(9)
    for t in (254, 100, 30, 6):
        a = guide.get_gradient(q, s, gl, t)
        b = og.get_gradient(q, s, gl, t)
        assert maxabs(a, b) <= 5e-5 and rmse(a, b) <= 3e-6, (t, maxabs(a, b), rmse(a, b))


@pytest.mark.parametrize("n_obstacles,bpg,guides", [(1, 1, [1]), (1, 2, [10, 13]), (64, 1, [1, 2, 3, 4, 5, 10]), (7, 1, [11, 18, 9])])
def test_guide_edge_sizes_vs_oracle(oracle, n_obstacles, bpg, guides):
    """one obstacle, the maximum number of obstacles (EDMP_MAX_OBSTACLES = 64), single-row batches, ragged trajectory
    lengths: costs, swept-volume costs, gradient and the best-row choice against the oracle."""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = cfgs_for(guides, bpg)
    B = cfgs["total_batch_size"]
    scene = scenes.random_scene(40 + n_obstacles, n_obstacles)
    guide = IntersectionVolumeGuide(scene, DEV, cfgs, B)
    og = oracle.GuideOracle(scene, cfgs, B)
    rs = np.random.RandomState(n_obstacles)
    lo, hi = oracle.joint_limits()
    s, gl = scenes.random_start_goal(3)
    for L in (48, 1, 5):
        q = oracle.clip_joints(rs.uniform(lo[None, :, None], hi[None, :, None], (B, 7, L)))
        for t in (0, 200, 6):
            if t == 0:
                qa = q[:1] if B > 1 else q  # t = 0 evaluates any number of rows against the un-inflated scene
                a = guide.cost(torch.tensor(qa), 0, batch_size=qa.shape[0]).cpu().numpy()
                b = og.cost(torch.tensor(qa, dtype=torch.float32), 0, batch_size=qa.shape[0]).numpy()
            else:
                a = guide.cost(torch.tensor(q), t).cpu().numpy()
                b = og.cost(torch.tensor(q, dtype=torch.float32), t).numpy()
            assert a.shape == b.shape and maxabs(a, b) <= 2e-6, (L, t, maxabs(a, b))
        if L >= 2:
            for t in (254, 6):
                a = guide.get_gradient(q, s, gl, t)
                b = og.get_gradient(q, s, gl, t)
                # a batch whose gradient is exactly zero (one small obstacle, nothing touches it) turns into NaN
                # everywhere in the reference (quirk Q7: g / ||g||): the NaN pattern must match too
                assert np.array_equal(np.isnan(a), np.isnan(b)), (L, t)
                fin = ~np.isnan(b)
                if fin.any():
                    assert maxabs(a[fin], b[fin]) <= 5e-5 and rmse(a[fin], b[fin]) <= 5e-6, (L, t, maxabs(a[fin], b[fin]))
    traj = oracle.clip_joints(rs.uniform(lo[None, :, None], hi[None, :, None], (B, 7, 50)))
    va, ia = guide.row_swept_volumes(s, gl, traj)
    vb = og.row_swept_volumes(s, gl, traj)
    assert maxabs(va, np.asarray(vb)) <= 2e-5 and ia == int(np.argmin(np.asarray(vb)))


@pytest.mark.parametrize("tag", ["c1_g1_b4", "c3_g6_b12", "mixed_b12", "full_b6"])
def test_teacher_forced_steps(golden, tiny_net, tag):
    """Every kept step of the reference's own run: feed its X_t and z_t, compare eps, posterior, gradient, X_{t-1}.
    `full_b6` is a run of the reference on the FULL dims=(32,64,128,256,512,512) network: its steps pass through the
    position-tile / whole-level kernels (wide_conv_kernel, level_kernel incl. the Karatsuba forms) that bench.py times."""
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide

    g = golden(f"g9_trace_{tag}")
    if "unet_dims" in g.files:
        from edmp_amd import weights as W
        from edmp_amd.temporalunet import TemporalUNet

        dims = tuple(int(d) for d in g["unet_dims"])
        assert dims == FULL_DIMS
        net = TemporalUNet(None, 7, 32, DEV, dims=dims, state_dict=W.init_state_dict(int(g["unet_seed"]), 7, 32, dims), max_batch=8)
    else:
        net, _ = tiny_net
    cfgs = cfgs_for(g["guides"], g["bpg"])
    B = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    noise = noise_for(g["seed"], B)
    worst = 0.0
    for t in g["steps"]:
        t = int(t)
        st = dif.denoise_step(net, guide, g[f"x_in_{t}"], noise[1 + (T - t)], t, g["start"], g["goal"], cfgs["guidance_schedule"])
        assert rmse(st["eps"], g[f"eps_{t}"]) <= 2e-5, (t, "eps")
        assert rmse(st["x_post"], g[f"x_post_{t}"]) <= 1e-6, (t, "x_post")
        if f"grad_{t}" in g.files:
            assert st["grad"] is not None
            assert rmse(st["grad"], g[f"grad_{t}"]) <= 1e-5, (t, "grad", rmse(st["grad"], g[f"grad_{t}"]))
        else:
            assert st["grad"] is None
        e = rmse(st["x_out"], g[f"x_out_{t}"])
        worst = max(worst, e)
        assert e <= 1e-4, (t, "x_out", e)  # the north-star tolerance
        assert np.array_equal(st["x_out"][:, :, 0], np.broadcast_to(g["start"], (B, 7)))
        assert np.array_equal(st["x_out"][:, :, -1], np.broadcast_to(g["goal"], (B, 7)))
    assert worst <= 2e-5, worst  # what we actually achieve


def test_forward_process_golden(golden):
    """q_sample / q_sample_from_x0 / generate_q_sample on the GPU == the reference's f64 outputs, bit for bit, with the
    global NumPy RNG consumed in the reference's order."""
    from edmp_amd.diffusion import Diffusion

    d = Diffusion(T, DEV)
    g = golden("g12_qsample")
    np.random.seed(int(g["gq_seed"]))
    X, Y, ts, means, vars_ = d.generate_q_sample(g["x0"].copy(), return_type="numpy")
    for a, k in ((X, "gq_X"), (Y, "gq_Y"), (ts, "gq_t"), (means, "gq_means"), (vars_, "gq_vars")):
        assert np.array_equal(a, g[k]), k
    np.random.seed(int(g["gq2_seed"]))
    X2, Y2, _, means2, vars2 = d.generate_q_sample(g["x0"].copy(), time_steps=g["gq2_t"], condition=False, return_type="numpy")
    for a, k in ((X2, "gq2_X"), (Y2, "gq2_Y"), (means2, "gq2_means"), (vars2, "gq2_vars")):
        assert np.array_equal(a, g[k]), k
    np.random.seed(int(g["gq3_seed"]))
    Xt, Yt, tt, _, _ = d.generate_q_sample(g["x0"].copy())
    assert Xt.dtype == torch.float32 and np.array_equal(Xt.numpy(), g["gq3_X32"]) and np.array_equal(Yt.numpy(), g["gq3_Y32"])
    assert np.array_equal(tt.numpy(), g["gq3_t32"])
    xs, ms, vs = d.q_sample(g["x0"], g["qs_t"], g["qs_eps"])
    assert np.array_equal(xs, g["qs_xt"]) and np.array_equal(ms, g["qs_mean"]) and np.array_equal(vs, g["qs_var"])
    np.random.seed(int(g["q0_seed"]))
    assert np.array_equal(d.q_sample_from_x0(g["x0"], g["qs_t"])[0], g["q0_xt"])
    # scalar timestep broadcast + error behaviour at the boundary
    x1, _, v1 = d.q_sample_from_x0(g["x0"], 255, g["qs_eps"])
    assert np.array_equal(x1, np.sqrt(d.alpha_bar[254]) * g["x0"] + np.sqrt(1 - d.alpha_bar[254]) * g["qs_eps"]) and v1.shape == (6, 1, 1)
    from edmp_amd._capi import EdmpError

    with pytest.raises(EdmpError, match="outside 1"):
        d.q_sample(g["x0"], 0, g["qs_eps"])
    with pytest.raises(EdmpError, match="outside 1"):
        d.q_sample(g["x0"], 256, g["qs_eps"])


def test_graph_replay_is_bit_identical(golden, tiny_net):
    """edmp_sampler_set_graph: the captured + replayed loop gives exactly the eager loop's trajectories, keeps doing so
    when start / goal change between replays, and re-captures when the scene or the rows change."""
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide

    net, _ = tiny_net
    g = golden("g9_trace_mixed_b12")
    cfgs = cfgs_for(g["guides"], g["bpg"])
    B = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    noise = dif.ctx.to_dev(noise_for(5, B), torch.float64)
    run = lambda s, e: dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=s, goal=e, noise=noise)  # noqa: E731
    goal2 = g["goal"] * 0.5
    eager = [run(g["start"], g["goal"]), run(g["start"], goal2)]
    dif.set_graph_replay(True)
    try:
        assert np.array_equal(run(g["start"], g["goal"]), eager[0])  # capture + first launch
        assert np.array_equal(run(g["start"], g["goal"]), eager[0])  # replay
        assert np.array_equal(run(g["start"], goal2), eager[1])      # replay with another goal (device-side start/goal)
        from edmp_amd import scenes

        scene2 = scenes.random_scene(3, 8)
        guide2 = IntersectionVolumeGuide(scene2, DEV, cfgs, B)        # new obstacle table: the graph must be re-captured
        got = dif.denoise_guided(net, guide2, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"], noise=noise)
    finally:
        dif.set_graph_replay(False)
    want = dif.denoise_guided(net, guide2, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"], noise=noise)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, eager[0])


def test_bitwise_determinism_and_stream_handover(golden, tiny_net):
    """No atomics, no races: repeated UNet forwards (full + ragged batches) and repeated guided loops are bit-identical,
    and a device tensor returned by denoise_guided(return_device=True) can be used on torch's current stream at once
    (the context orders the caller's stream after its own)."""
    from edmp_amd import _capi
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import ptr
    from edmp_amd.temporalunet import TemporalUNet

    net = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, seed=3, max_batch=256)
    ctx = net.ctx
    for B in (256, 77, 3):
        x = ctx.to_dev(torch.randn(B, 7, 50, generator=torch.Generator().manual_seed(B)), torch.float32)
        eps = ctx.empty(x.shape, torch.float32)
        ref = None
        for i in range(40):
            _capi.check(ctx.lib.edmp_unet_forward_dev(ctx.h, ptr(x), B, 100, ptr(eps)))
            cur = ctx.hand_over(eps).clone()  # clone runs on torch's current stream
            ref = cur if ref is None else ref
            assert torch.equal(cur, ref), (B, i)
    tiny, _ = tiny_net
    g = golden("g9_trace_mixed_b12")
    cfgs = cfgs_for(g["guides"], g["bpg"])
    B = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    noise = torch.from_numpy(noise_for(9, B)).to(DEV)  # made on the caller's stream: the context must adopt it
    ref = None
    for i in range(4):
        X = dif.denoise_guided(tiny, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"], noise=noise, return_device=True)
        cur = (X + 0.0).cpu().numpy()  # default-stream op right after the call
        ref = cur if ref is None else ref
        assert np.array_equal(cur, ref), i
    assert np.array_equal(ref, dif.denoise_guided(tiny, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"], noise=noise_for(9, B)))


def test_free_running_unguided(oracle, tiny_net):
    """guide off: the loop is contractive, so 255 free-running steps must track the oracle."""
    from edmp_amd.diffusion import Diffusion

    net, sd = tiny_net
    dif = Diffusion(T, DEV)
    B = 5
    noise = noise_for(77, B)
    from edmp_amd import scenes

    X = dif.denoise_guided(net, None, 50, 7, None, batch_size=B, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL, noise=noise)

    class NoGuide:
        def get_gradient(self, q, s, g, t):
            return np.zeros_like(q)

    Xo = oracle.denoise_guided(oracle.UNetOracle(sd), NoGuide(), T, 50, 7, np.zeros((B, T)), B, scenes.DEFAULT_START, scenes.DEFAULT_GOAL, noise=noise)
    assert rmse(X, Xo) <= 1e-4, rmse(X, Xo)


def test_chunked_numpy_stream_equals_resident_stream(golden, tiny_net):
    """noise=None draws NumPy's global stream in chunks while the GPU works (segmented loop): same numbers, same result
    as uploading the whole (T+1,B,7,50) stream first — for chunk sizes that do and do not divide T."""
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide

    net, _ = tiny_net
    g = golden("g9_trace_mixed_b12")
    cfgs = cfgs_for(g["guides"], g["bpg"])
    B = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    Xr = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"], noise=noise_for(31, B))
    for chunk in (16, 7, 255, 1000):
        np.random.seed(31)
        Xc = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"], chunk_steps=chunk)
        assert np.array_equal(Xc, Xr), chunk
    # the RNG is left exactly where the reference leaves it: (T + 1) * B * 7 * 50 normals consumed
    np.random.seed(31)
    dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"])
    after = np.random.standard_normal(3)
    np.random.seed(31)
    np.random.standard_normal((T + 1, B, 7, 50))
    assert np.array_equal(after, np.random.standard_normal(3))
    # a run that stops early draws X_T and the 21 steps it takes, nothing more: 22 * B * 7 * 50 normals
    kw = dict(batch_size=B, start=g["start"], goal=g["goal"])
    stream = noise_for(31, B)
    Xs = {0: Xr, T - 21: dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], noise=stream, t_stop=T - 21, **kw)}
    assert not np.array_equal(Xs[0], Xs[T - 21])
    np.random.seed(31)
    Xc = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], chunk_steps=7, t_stop=T - 21, **kw)
    after = np.random.standard_normal(3)
    assert np.array_equal(Xc, Xs[T - 21])
    np.random.seed(31)
    np.random.standard_normal((22, B, 7, 50))
    assert np.array_equal(after, np.random.standard_normal(3))
    # the same stream in page-locked host memory, whole or handed over as a (fully published) stream that is being drawn
    from edmp_amd.diffusion import PinnedNoiseStream

    pinned = torch.from_numpy(stream).pin_memory()
    for chunk in (16, 7):
        for t_stop in (0, T - 21):
            for as_stream in (False, True):
                z = pinned
                if as_stream:
                    z = PinnedNoiseStream(pinned)
                    z.publish(pinned.numel())
                Xp = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], noise=z, chunk_steps=chunk, t_stop=t_stop, **kw)
                assert np.array_equal(Xp, Xs[t_stop]), (chunk, t_stop, as_stream)


def test_condition_false(oracle, tiny_net):
    """`condition=False` (diffusion.py:305, 347): no start/goal pinning."""
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion

    net, sd = tiny_net
    dif = Diffusion(T, DEV)
    B = 3
    noise = noise_for(78, B)
    s, g = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    X = dif.denoise_guided(net, None, 50, 7, None, batch_size=B, start=s, goal=g, condition=False, noise=noise)

    class NoGuide:
        def get_gradient(self, q, s, g, t):
            return np.zeros_like(q)

    Xo = oracle.denoise_guided(oracle.UNetOracle(sd), NoGuide(), T, 50, 7, np.zeros((B, T)), B, s, g, noise=noise, condition=False)
    assert rmse(X, Xo) <= 1e-4, rmse(X, Xo)
    assert not np.allclose(X[:, :, 0], s)
    Xc = dif.denoise_guided(net, None, 50, 7, None, batch_size=B, start=s, goal=g, condition=True, noise=noise)
    assert np.array_equal(Xc[:, :, 0], np.broadcast_to(s, (B, 7)))


def test_free_running_guided_envelope(golden, tiny_net):
    """guided loop is chaotic: report RMSE vs the reference's own run, gate only sanity + iv rows."""
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide

    net, _ = tiny_net
    g = golden("g9_trace_c1_g1_b4")
    cfgs = cfgs_for(g["guides"], g["bpg"])
    B = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    np.random.seed(int(g["seed"]))
    X = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"], condition=True, benchmarking=True)
    assert X.shape == (B, 7, 50) and X.dtype == np.float64 and np.isfinite(X).all()
    e = rmse(X, g["X_final"])
    print(f"\nfree-running guided RMSE vs reference run: {e:.3e} (reference's own 1e-7-perturbation envelope ~0.9 rad)")
    assert e < 3.0
    # same first 3 steps when stopped early (deterministic prefix)
    X3 = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"], noise=noise_for(g["seed"], B), t_stop=T - 3)
    assert rmse(X3, g["x_out_253"]) <= 1e-4


def test_best_trajectory(golden):
    from edmp_amd.guide import IntersectionVolumeGuide

    for tag in ("c1_g1_b4", "c3_g6_b12", "mixed_b12"):
        g = golden(f"g9_trace_{tag}")
        cfgs = cfgs_for(g["guides"], g["bpg"])
        guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, cfgs["total_batch_size"])
        vols, idx = guide.row_swept_volumes(g["start"], g["goal"], g["X_final"])
        assert np.allclose(vols, g["row_volumes"], rtol=2e-5, atol=1e-6), tag
        assert idx == int(g["best_index"])
        assert np.array_equal(guide.choose_best_trajectory(g["start"], g["goal"], g["X_final"]), g["best"])


def test_full_size_properties():
    """B = 1024, full-size UNet, 6-guide ensemble: size-independent properties (determinism, conditioning,
    row independence of the denoiser, batch-split invariance of the guided step)."""
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.guide_cfg import split_rows
    from edmp_amd.temporalunet import TemporalUNet

    B = 1024
    net = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, seed=1, max_batch=B)
    guides = [1, 2, 3, 4, 5, 10]
    cfgs = cfgs_for(guides, 0, rows_per_guide=split_rows(B, len(guides)))
    scene = scenes.random_scene(11, 16)
    guide = IntersectionVolumeGuide(scene, DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    rs = np.random.RandomState(3)
    noise = rs.standard_normal((T + 1, B, 7, 50))
    s, gl = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    # 8 steps incl. 4 guided ones
    X1 = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=s, goal=gl, noise=noise, t_stop=T - 8)
    X2 = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=s, goal=gl, noise=noise, t_stop=T - 8)
    assert np.array_equal(X1, X2), "run-to-run determinism"
    assert np.isfinite(X1).all()
    assert np.array_equal(X1[:, :, 0], np.broadcast_to(s, (B, 7))) and np.array_equal(X1[:, :, -1], np.broadcast_to(gl, (B, 7)))
    # the denoiser treats rows independently: a 100-row slice gives the same eps as inside the 1024 batch
    x = torch.tensor(noise[0], dtype=torch.float32)
    e_all = net(x, torch.tensor([200.0])).cpu().numpy()
    e_sub = net(x[300:400], torch.tensor([200.0])).cpu().numpy()
    assert np.array_equal(e_all[300:400], e_sub)


def test_device_loop_equals_the_stepwise_api_at_full_size():
    """The device-resident loop runs the tail of a reverse step (final 1x1 conv, posterior, conditioning, next input)
    inside the UNet's last launch (level kernel, tail.h); the stepwise API runs it as its own launch.  Same code, same
    operands: the state after 6 steps (3 guided) must be bit-identical, rows of a ragged last workgroup included."""
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.guide_cfg import split_rows
    from edmp_amd.temporalunet import TemporalUNet

    B = 37  # not a multiple of the level kernel's 4-sample workgroups
    net = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, seed=2, max_batch=64)
    guides = [1, 10, 11]
    cfgs = cfgs_for(guides, 0, rows_per_guide=split_rows(B, len(guides)))
    scene = scenes.random_scene(5, 12)
    guide = IntersectionVolumeGuide(scene, DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    noise = np.random.RandomState(8).standard_normal((T + 1, B, 7, 50))
    s, gl = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    n = 6
    X_loop = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=s, goal=gl, noise=noise, t_stop=T - n)
    X = noise[0].copy()
    X[:, :, 0], X[:, :, -1] = s, gl
    for k, t in enumerate(range(T, T - n, -1)):
        X = dif.denoise_step(net, guide, X, noise[1 + k], t, s, gl, cfgs["guidance_schedule"])["x_out"]
    assert np.array_equal(X_loop, X), (float(np.abs(X_loop - X).max()), int((X_loop != X).sum()), np.argwhere(X_loop != X)[:5].tolist())
    # the same with the device noise source (Philox inside the fused tail) against the materialised stream
    Xd = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=s, goal=gl, noise="device", seed=77, t_stop=T - n)
    stream = np.zeros((T + 1, B, 7, 50))
    for k in range(n + 1):
        stream[k] = dif.device_noise(77, k, B)
    Xs = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=s, goal=gl, noise=stream, t_stop=T - n)
    assert np.array_equal(Xd, Xs)


def test_infer_serial_driver_c1():
    """BASELINE configs[0] plumbing: guides [1], 4 rows, one scene, through the reference-shaped driver."""
    import os

    import infer_serial

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = infer_serial.run(os.path.join(root, "configs", "cfg_c1_plumbing.yaml"), verbose=False)
    assert len(res) == 1 and res[0]["trajectory"].shape == (7, 50) and np.isfinite(res[0]["trajectory"]).all()
    assert res[0]["rows"] == 4 and 0 <= res[0]["rows_ok"] <= 4 and res[0]["success_proxy"] in (0, 1)
    # a dataset that hands cuboids AND cylinders (fetch_data contract of datasets/load_test_dataset.py:76-189): the driver marks
    # the cylinder rows for the success check (infer_serial.py:159-163 spawns them as true cylinders); flags = the checker's
    from edmp_amd import scenes
    from oracle import success_oracle as SO

    ds = scenes.SyntheticDataset(scene_types=("stress",), n_obstacles=6, n_cylinders=2)
    res = infer_serial.run(os.path.join(root, "configs", "cfg_c1_plumbing.yaml"), dataset=ds, verbose=False)
    oc = ds.fetch_data(0, "stress")[0]
    ref = SO.success_rows(res[0]["trajectory"][None], oc, kinds=np.array([0, 0, 0, 0, 1, 1]))
    # the driver tallies the REFERENCE's flag (no contact; lib/environment.py:672) and reports the strict one (also inside the limits) beside it
    assert res[0]["success_proxy"] == int(ref["first"][0] < 0) and res[0]["success_strict"] == int(ref["ok"][0]) and res[0]["first_collision_waypoint"] == int(ref["first"][0])
    assert res[0]["rows_ok"] <= res[0]["rows_collision_free"] <= res[0]["rows"]


def test_infer_serial_on_a_converted_problem_set(tmp_path):
    """a problem-set JSON in the format scripts/mpinets_pkl_to_json.py writes from an MPiNets pickle (cuboids +
    true cylinders, quaternions w-first, goals as an explicit input) drives the reference-shaped scene loop through
    scenes.ProblemSetDataset; the success check sees the cylinders as cylinders.  (The pickle -> JSON half is a CPU test.)"""
    import json
    import os

    import yaml

    import infer_serial
    from edmp_amd import franka, scenes
    from oracle import success_oracle as SO

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lo, hi = franka.joint_limits()
    rs = np.random.RandomState(9)
    problems = []
    for k in range(2):
        oc = scenes.random_scene(20 + k, 6)
        to_wxyz = lambda o: [float(o[6]), float(o[3]), float(o[4]), float(o[5])]  # noqa: E731
        problems.append({"cuboids": [{"center": o[:3].tolist(), "quaternion_wxyz": to_wxyz(o), "dims": o[7:10].tolist()} for o in oc[:4]],
                         "cylinders": [{"center": o[:3].tolist(), "quaternion_wxyz": to_wxyz(o), "radius": float(o[7]), "height": float(o[9])} for o in oc[4:]],
                         "start": rs.uniform(lo, hi).tolist(), "target": {"xyz": [0.4, 0.0, 0.4], "quaternion_wxyz": [0, 1, 0, 0], "frame": "right_gripper"},
                         "goals": rs.uniform(lo, hi, (20, 7)).tolist()})
    pj = tmp_path / "problems.json"
    json.dump({"format": "edmp_amd problem set v1", "scene_types": {"tabletop": problems}}, open(pj, "w"))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "cfg_c1_plumbing.yaml")))
    cfg["dataset"]["scene_types"] = ["tabletop"]
    os.makedirs(tmp_path / "cfgs")
    cj = tmp_path / "cfgs" / "cfg_problem_set.yaml"
    yaml.safe_dump(cfg, open(cj, "w"))
    ds = scenes.ProblemSetDataset(str(pj))
    res = infer_serial.run(str(cj), dataset=ds, verbose=False)
    # ... and through the run config alone, the way the reference selects its dataset (dataset_type 'global' + path,
    # datasets/load_test_dataset.py:15-38): <path>/global_solvable_problems.json is picked up
    import shutil

    shutil.copy(pj, tmp_path / "global_solvable_problems.json")
    cfg["dataset"]["dataset_type"], cfg["dataset"]["path"] = "global", str(tmp_path)
    cg = tmp_path / "cfgs" / "cfg_global.yaml"
    yaml.safe_dump(cfg, open(cg, "w"))
    np.random.seed(123)
    res_a = infer_serial.run(str(cg), verbose=False)
    np.random.seed(123)
    res_b = infer_serial.run(str(cj), dataset=ds, verbose=False)
    assert all(np.array_equal(a["trajectory"], b["trajectory"]) for a, b in zip(res_a, res_b))
    assert len(res) == 2 and all(r["scene_type"] == "tabletop" and np.isfinite(r["trajectory"]).all() for r in res)
    for k, r in enumerate(res):
        oc = ds.fetch_data(k, "tabletop")[0]
        ref = SO.success_rows(r["trajectory"][None], oc, kinds=np.array([0, 0, 0, 0, 1, 1]))
        assert r["success_proxy"] == int(ref["first"][0] < 0) and r["first_collision_waypoint"] == int(ref["first"][0])
        assert np.array_equal(r["trajectory"][:, 0], np.asarray(problems[k]["start"]))  # conditioned on the problem's own start


def test_infer_serial_two_scenes_in_flight():
    """the driver with two scenes planned concurrently on one GPU (two contexts, two host threads) returns, scene by scene, what
    the serial loop returns under the same np.random seed - bit for bit (noise drawn per scene, in scene order, on the caller's thread)."""
    import os

    import infer_serial
    from edmp_amd import scenes

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = os.path.join(root, "configs", "cfg_c1_plumbing.yaml")
    out = []
    for k in (1, 2):
        np.random.seed(77)
        ds = scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=3, n_obstacles=6, n_cylinders=1)
        out.append(infer_serial.run(cfg, dataset=ds, verbose=False, scenes_in_flight=k))
    assert len(out[0]) == len(out[1]) == 3
    for a, b in zip(*out):
        assert (a["scene_num"], a["best_row"], a["success_proxy"], a["rows_ok"]) == (b["scene_num"], b["best_row"], b["success_proxy"], b["rows_ok"])
        assert np.array_equal(a["trajectory"], b["trajectory"])
    assert not np.array_equal(out[0][0]["trajectory"], out[0][1]["trajectory"])  # different scenes, different noise


def test_infer_serial_noise_is_the_reference_contract_stream():
    """The scene loop's noise comes from a feeder thread that draws every scene's stream a scene ahead into page-locked memory, piece by
    piece, uploaded chunk by chunk (round 6).  It must be exactly what the reference's loop would see: scene k's trajectories equal a direct
    denoise_guided call on the SAME scene whose (T+1, B, 7, 50) noise is NumPy's own np.random.standard_normal draw number k after the seed
    (diffusion.py:303, 126: X_T first, then one draw per step - one contiguous stream per scene)."""
    import os

    import infer_serial
    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.temporalunet import TemporalUNet

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg_path = os.path.join(root, "configs", "cfg_c1_plumbing.yaml")
    np.random.seed(123)
    ds = scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=2, n_obstacles=6, n_cylinders=1)
    res = infer_serial.run(cfg_path, dataset=ds, verbose=False, scenes_in_flight=1)
    cfg = GC.load_yaml(cfg_path)
    guide_cfgs = GC.guide_cfgs_from_run_cfg(cfg, base_dir=os.path.dirname(os.path.abspath(cfg_path)) + "/..")
    B, Tm, N, Cc = guide_cfgs["total_batch_size"], cfg["model"]["T"], cfg["model"]["traj_len"], cfg["model"]["num_channels"]
    net = TemporalUNet(model_name=None, input_dim=Cc, time_dim=32, dims=(32, 64, 128, 256, 512, 512), device=DEV, max_batch=B)
    dif = Diffusion(T=Tm, device=DEV)
    np.random.seed(123)
    for k, r in enumerate(res):
        obstacle_config, _, _, ncub, ncyl, start, ik_goals = ds.fetch_data(scene_num=r["scene_num"], scene_type=r["scene_type"])
        noise = np.random.standard_normal((Tm + 1, B, Cc, N))  # NumPy itself, one call per scene, in scene order
        kinds = np.concatenate([np.zeros(int(ncub), dtype=np.int32), np.ones(int(ncyl), dtype=np.int32)])
        guide = IntersectionVolumeGuide(obstacle_config=obstacle_config, device=DEV, guide_cfgs=guide_cfgs, batch_size=B, obstacle_kinds=kinds)
        vol = guide.cost(torch.tensor(ik_goals.reshape((-1, 7, 1))), 0, batch_size=ik_goals.shape[0]).sum(axis=(1, 2)).cpu().numpy()
        idx = np.argsort(vol)
        goals = ik_goals[idx][vol[idx] < np.min(vol) + 0.0008]
        goal = goals[np.argmin(np.linalg.norm(start - goals, axis=1))]
        X = dif.denoise_guided(net, guide, N, Cc, guide_cfgs["guidance_schedule"], batch_size=B, start=start, goal=goal, noise=noise)
        assert np.array_equal(X[r["best_row"]], r["trajectory"]), k


def test_infer_serial_scene_sharded_over_two_ranks(tmp_path):
    """the reference-shaped driver under `python -m torch.distributed.run --nproc-per-node 2` (one process per GPU; gloo over the
    one GPU of a test box, RCCL with two): scene i goes to rank i mod 2, nothing is exchanged until the tallies are summed, and
    rank 0's first scene is what a single-process run plans first under the same seed."""
    import json
    import os
    import socket
    import subprocess
    import sys

    import yaml

    import infer_serial
    from tests.conftest import ROOT

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cfg_c1_plumbing.yaml")))
    cfg["dataset"]["num_scenes_per_type"] = 3
    os.makedirs(tmp_path / "cfgs")
    cj = tmp_path / "cfgs" / "cfg_three_scenes.yaml"
    yaml.safe_dump(cfg, open(cj, "w"))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if torch.cuda.device_count() < 2:
        env["EDMP_DIST_BACKEND"] = "gloo"
    out = tmp_path / "res.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "infer_serial.py"), "-c", str(cj), "--seed", "5", "--results-json", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d0, d1 = json.load(open(out)), json.load(open(str(out) + ".rank1"))
    assert [x["scene_num"] for x in d0["scenes"]] == [0, 2] and [x["scene_num"] for x in d1["scenes"]] == [1]
    sm = d0["summary"]
    assert sm == d1["summary"] and sm["ranks"] == 2 and sm["scenes"] == 3 and sm["scenes_per_rank"] == [2, 1] and sm["rows"] == 12
    assert sm["success_proxy"] == sum(x["success_proxy"] for x in d0["scenes"] + d1["scenes"])
    assert "3 scenes on 2 rank(s)" in r.stdout
    np.random.seed(5)
    one = infer_serial.run(str(cj), verbose=False, max_scenes=1)
    a, b = one[0], d0["scenes"][0]
    assert (a["best_row"], a["success_proxy"], a["rows_collision_free"]) == (b["best_row"], b["success_proxy"], b["rows_collision_free"]) and a["swept_volume"] == b["swept_volume"]


def test_device_noise_mode(tiny_net):
    """noise="device" (Philox on the GPU, explicitly non-parity): statistics of the stream, determinism, seed / step
    independence, and the loop driven by it equals the loop driven by the materialised stream."""
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide

    net, _ = tiny_net
    dif = Diffusion(T, DEV)
    B = 64
    z = np.stack([dif.device_noise(7, s, B) for s in range(40)])  # 40 x 64 x 7 x 50 = 896k samples
    assert abs(z.mean()) < 5e-3 and abs(z.var() - 1.0) < 1e-2
    assert abs(np.mean(z**3)) < 2e-2 and abs(np.mean(z**4) - 3.0) < 6e-2
    assert np.abs(z).max() < 7.0
    # no correlation between channels / steps / neighbours
    assert abs(np.corrcoef(z[:, :, 0].ravel(), z[:, :, 1].ravel())[0, 1]) < 1e-2
    assert abs(np.corrcoef(z[0].ravel(), z[1].ravel())[0, 1]) < 2e-2
    assert abs(np.corrcoef(z[..., :-1].ravel(), z[..., 1:].ravel())[0, 1]) < 5e-3
    assert np.array_equal(dif.device_noise(7, 3, B), z[3])  # deterministic
    assert not np.allclose(dif.device_noise(8, 3, B), z[3])  # seed matters
    # the fused loop with the device source == the loop fed the same numbers as an explicit stream
    cfgs = cfgs_for([1, 10], 3)
    Bg = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(scenes.random_scene(5, 8), DEV, cfgs, Bg)
    s, g = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    Xd = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=Bg, start=s, goal=g, noise="device", seed=123, t_stop=T - 12)
    stream = np.zeros((T + 1, Bg, 7, 50))
    for k in range(13):
        stream[k] = dif.device_noise(123, k, Bg)
    Xs = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=Bg, start=s, goal=g, noise=stream, t_stop=T - 12)
    assert np.array_equal(Xd, Xs)
    Xfull = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=Bg, start=s, goal=g, noise="device", seed=5)
    assert np.isfinite(Xfull).all() and np.array_equal(Xfull[:, :, 0], np.broadcast_to(s, (Bg, 7)))


def test_plain_c_host_through_the_c_abi(golden, tmp_path):
    """tests/c_abi/c_abi_smoke.c: a C program (gcc, no Python, no torch) binds include/edmp_hip.h, runs 3 guided
    reverse steps of the reference's own run (golden trace) and picks the best row.  Same numbers as the Python path,
    and within the north-star tolerance of the reference."""
    import os
    import struct
    import subprocess

    from edmp_amd import franka
    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide, row_classes
    from edmp_amd.temporalunet import TemporalUNet

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "c_abi", "c_abi_smoke")
    if not os.path.exists(exe):  # normally prebuilt by __graft_entry__.build(); compile here otherwise (plain gcc)
        exe = str(tmp_path / "c_abi_smoke")
        subprocess.run(["gcc", "-O2", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(root, "include"),
                        os.path.join(root, "tests", "c_abi", "c_abi_smoke.c"), "-o", exe, "-L" + os.path.join(root, "edmp_amd"), "-ledmp_hip",
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(root, "edmp_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    g = golden("g9_trace_mixed_b12")
    cfgs = cfgs_for(g["guides"], g["bpg"])
    B = cfgs["total_batch_size"]
    sd = W.init_state_dict(5, 7, 32, TINY_DIMS)
    flat = np.concatenate([np.asarray(sd[k], dtype=np.float32).reshape(-1) for k in W.unet_param_shapes(7, 32, TINY_DIMS)])
    rc, cclr, cexp = row_classes(cfgs["clearance"], cfgs["expansion"])
    noise = noise_for(g["seed"], B)
    t_stop = T - 3
    blob = struct.pack("<6i", B, g["scene"].shape[0], cclr.shape[0], T, flat.size, t_stop)
    for arr, dt in ((flat, np.float32), (g["scene"], np.float64), (cclr, np.float64), (cexp, np.float64), (franka.link_half_extents(), np.float32),
                    (franka.dh_table(), np.float32), (franka.static_frames(), np.float32), (rc, np.int32), (cfgs["guidance_method"], np.float32),
                    (cfgs["grad_norm"], np.float64), (cfgs["guidance_schedule"], np.float64), (g["start"], np.float64), (g["goal"], np.float64),
                    (noise, np.float64)):
        blob += np.ascontiguousarray(arr, dtype=dt).tobytes()
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(blob)
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = fout.read_bytes()
    n = B * 7 * 50
    Xc = np.frombuffer(raw[: n * 8], dtype=np.float64).reshape(B, 7, 50)
    best = struct.unpack("<i", raw[n * 8 : n * 8 + 4])[0]
    vols = np.frombuffer(raw[n * 8 + 4 : n * 8 + 4 + 4 * B], dtype=np.float32)
    tail = np.frombuffer(raw[n * 8 + 4 + 4 * B :], dtype=np.int32)
    flags, counts = tail[: 3 * B].reshape(3, B), tail[3 * B :]
    assert rmse(Xc, g["x_out_253"]) <= 1e-4, rmse(Xc, g["x_out_253"])
    # the success check through the plain-C host (last obstacle a true cylinder; dh_f64 = NULL: the widened f32 table) equals
    # the Python mirror's flags on the same state
    from oracle import success_oracle as SO

    kinds = np.zeros(g["scene"].shape[0], dtype=np.int32)
    kinds[-1] = 1
    ref = SO.success_rows(Xc, g["scene"], kinds=kinds)
    assert np.array_equal(flags[0].astype(bool), ref["ok"]) and np.array_equal(flags[1], ref["first"]) and np.array_equal(flags[2].astype(bool), ref["within"])
    assert counts.tolist() == [int(ref["ok"].sum()), int(ref["within"].sum()), int((ref["first"] < 0).sum()), B]
    # identical to the Python mirror (same library underneath)
    net = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=sd, max_batch=B)
    guide = IntersectionVolumeGuide(g["scene"], DEV, cfgs, B)
    Xp = Diffusion(T, DEV).denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=g["start"], goal=g["goal"], noise=noise, t_stop=t_stop)
    assert np.array_equal(Xc, Xp)
    vp, ip = guide.row_swept_volumes(g["start"], g["goal"], Xp)
    assert best == ip and np.array_equal(vols, vp)


def _subset_cfgs(cfgs, rows):
    out = dict(cfgs)
    for k in ("clearance", "expansion", "guidance_method", "grad_norm", "guidance_schedule", "volume_trust_region"):
        out[k] = np.ascontiguousarray(np.asarray(cfgs[k])[rows])
    out["total_batch_size"] = len(rows)
    return out


def _tie_margins(oracle, scene, cfgs, rows, q_rows, start, goal, t, ref_grad_rows):
    """For rows whose HIP gradient differs from the oracle's by more than the tolerance: the smallest joint perturbation
    delta (rad) at which the ORACLE's own f32-autograd gradient of that row jumps by more than the tolerance.  The
    overlap-volume cost is piecewise smooth (arg-min/arg-max box corners, min/max of AABB faces, clamp at 0:
    lib/guide.py:361-395, 507-537); a jump under a 1e-6 rad perturbation (link corners move <= ~1e-6 m, the size of the
    float32 rounding envelope of the 7-joint FK chain) means the reference itself sits on a tie there - which branch
    carries the gradient is decided by the last ulps of sin/cos and the FMA order, on any platform."""
    go = oracle.GuideOracle(scene, _subset_cfgs(cfgs, rows), len(rows))
    rs = np.random.RandomState(12345)
    margins = np.full(len(rows), np.inf)
    for delta in (1e-7, 3e-7, 1e-6, 3e-6, 1e-5):
        for _ in range(12):
            pert = q_rows + delta * rs.choice([-1.0, 1.0], size=q_rows.shape)
            g = go.raw_gradient(pert, start, goal, t)
            jump = np.abs(g - ref_grad_rows).reshape(len(rows), -1).max(axis=1) > 1e-4
            margins = np.where(jump & np.isinf(margins), delta, margins)
        if np.all(np.isfinite(margins)):
            break
    return margins


FULL_SIZE_CASES = [
    # BASELINE config 3 (and 4's per-rank workload): every break-point of the schedules - first step, maximum inflation,
    # guide 10's expansion segments [80,255) / [20,80), guide 5's clearance ramp, an odd (unguided) step, the last guided step
    ("c3_six_guides", [1, 2, 3, 4, 5, 10], (255, 254, 200, 129, 128, 80, 20, 6)),
    # BASELINE config 2 as written
    ("c2_three_guides", [1, 2, 3], (254, 80)),
    # BASELINE config 5's guide list: 11 and 13 are grad_norm rows -> the whole-batch sum(g^2) at full size
    ("c5_eight_guides", [1, 2, 3, 4, 5, 10, 11, 13], (254, 128, 6)),
]


@pytest.mark.parametrize("tag,guides,steps", FULL_SIZE_CASES, ids=[c[0] for c in FULL_SIZE_CASES])
def test_teacher_forced_vs_oracle_at_full_size(oracle, tag, guides, steps):
    """BASELINE configs[1..4] sizes: B = 1024, full 29.9 M-parameter UNet, 16 obstacles.  For every listed reverse step t
    the state X_t is produced by the HIP path itself (free-running from t = 255 with device-resident noise), then ONE
    step is computed by both sides from that identical (X_t, z_t): eps, posterior, mixed gradient, X_{t-1} at the
    north-star tolerance.  Rows whose gradient differs are accepted only with proof, from the oracle side, that the
    reference is discontinuous there (a tie, _tie_margins) - a row that differs without a tie fails the test."""
    from edmp_amd import scenes
    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.guide_cfg import split_rows
    from edmp_amd.temporalunet import TemporalUNet

    B = 1024
    sd = W.init_state_dict(1, 7, 32, FULL_DIMS)
    net = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=B)
    cfgs = cfgs_for(guides, 0, rows_per_guide=split_rows(B, len(guides)))
    scene = scenes.random_scene(11, 16)
    guide = IntersectionVolumeGuide(scene, DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    s, gl = scenes.DEFAULT_START, scenes.DEFAULT_GOAL
    noise = np.random.RandomState(3).standard_normal((T + 1, B, 7, 50))
    om, og = oracle.UNetOracle(sd), oracle.GuideOracle(scene, cfgs, B)
    sched = oracle.schedule(T)
    n_flipped, worst_margin, record = 0, 0.0, []
    for t in steps:
        if t == T:
            X = np.array(noise[0])
            X[:, :, 0], X[:, :, -1] = s, gl
        else:
            X = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=s, goal=gl, noise=noise, t_stop=t)
        assert np.isfinite(X).all(), t
        z = noise[1 + (T - t)]
        ref = oracle.denoise_step(om, og, X, z, t, cfgs["guidance_schedule"], s, gl, sched)
        st = dif.denoise_step(net, guide, X, z, t, s, gl, cfgs["guidance_schedule"])
        scale = max(1.0, float(np.sqrt(np.mean(ref["eps"] ** 2))))  # random-init weights: |eps| grows along the run
        assert rmse(st["eps"], ref["eps"]) <= 2e-5 * scale, (tag, t, rmse(st["eps"], ref["eps"]), scale)
        assert rmse(st["x_post"], ref["x_post"]) <= 1e-6 * scale, (tag, t)
        record.append({"tag": tag, "step": int(t), "guided": ref["grad"] is not None, "flipped": 0, "worst_margin": 0.0,
                       "eps_rmse": rmse(st["eps"], ref["eps"]), "eps_rms_scale": scale, "x_out_rmse_all_rows": rmse(st["x_out"], ref["x_out"])})
        if ref["grad"] is None:
            assert st["grad"] is None
            assert rmse(st["x_out"], ref["x_out"]) <= 1e-4, (tag, t, rmse(st["x_out"], ref["x_out"]))
            continue
        # mixed gradients share the whole-batch norm when grad_norm rows exist: compare the RAW per-row gradient decision
        # through the mixed one of rows without grad_norm, and all rows after accounting for flips
        d = np.abs(st["grad"] - ref["grad"]).reshape(B, -1).max(axis=1)
        gmag = np.abs(ref["grad"]).reshape(B, -1).max(axis=1)
        flipped = np.flatnonzero(d > 1e-4 + 1e-5 * gmag)
        ok = np.ones(B, dtype=bool)
        ok[flipped] = False
        if len(flipped):
            assert len(flipped) <= 0.005 * B, f"{tag} t={t}: {len(flipped)} of {B} rows differ"
            q = oracle.clip_joints(ref["x_post"][:, :, 1:-1])[flipped]
            sub = oracle.GuideOracle(scene, _subset_cfgs(cfgs, flipped), len(flipped))
            raw_ref = sub.raw_gradient(q, s, gl, t)
            margins = _tie_margins(oracle, scene, cfgs, flipped, q, s, gl, t, raw_ref)
            assert np.all(margins <= 3e-6), f"{tag} t={t}: rows {flipped[margins > 3e-6]} differ from the oracle without a tie (margins {margins})"
            n_flipped += len(flipped)
            worst_margin = max(worst_margin, float(margins.max()))
            record[-1].update(flipped=int(len(flipped)), worst_margin=float(margins.max()), rows=[int(r) for r in flipped])
        assert rmse(st["grad"][ok], ref["grad"][ok]) <= 1e-5 * max(1.0, float(np.median(gmag))), (tag, t)
        assert rmse(st["x_out"][ok], ref["x_out"][ok]) <= 1e-4, (tag, t, rmse(st["x_out"][ok], ref["x_out"][ok]))
        assert np.median(np.abs(st["x_out"] - ref["x_out"]).reshape(B, -1).max(axis=1)) <= 1e-5
    print(f"[{tag}] steps {steps}: {n_flipped} tie-flipped row-steps, largest tie margin {worst_margin:.1e} rad")
    # the accepted tie flips, on record: gpurun merges gpurun_out/ back, the round commits the file under profiles/
    import json

    from tests.conftest import ROOT

    out_dir = os.path.join(ROOT, "gpurun_out", "parity_records")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"teacher_forced_full_size_{tag}.json"), "w") as f:
        json.dump({"test": "test_teacher_forced_vs_oracle_at_full_size", "B": B, "accept": "<= 0.5 % rows per step, each with an oracle-side tie margin <= 3e-6 rad",
                   "flipped_row_steps": n_flipped, "worst_margin": worst_margin, "steps": record}, f, indent=1)


def test_error_behaviour_through_the_boundary():
    """bad arguments are reported as EdmpError with the library's message; nothing crashes or silently falls back."""
    from edmp_amd import _capi, scenes
    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.temporalunet import TemporalUNet

    sd = W.init_state_dict(5, 7, 32, TINY_DIMS)
    net = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=sd, max_batch=4)
    with pytest.raises(_capi.EdmpError, match="max_batch"):
        net(torch.zeros(5, 7, 50), torch.tensor([3.0]))
    with pytest.raises(_capi.EdmpError, match="outside 1..T"):
        net(torch.zeros(2, 7, 50), torch.tensor([256.0]))
    with pytest.raises(ValueError):
        net(torch.zeros(2, 7, 50), torch.tensor([3.5]))
    with pytest.raises(ValueError):
        net(torch.zeros(2, 6, 50), torch.tensor([3.0]))
    bad = dict(sd)
    bad["final_conv.1.weight"] = np.zeros((7, 16, 2), dtype=np.float32)
    with pytest.raises(ValueError):
        TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=bad)
    with pytest.raises(KeyError):
        TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict={k: v for k, v in sd.items() if "final_conv" not in k})
    cfgs = cfgs_for([1, 10], 2)
    with pytest.raises(ValueError):
        IntersectionVolumeGuide(np.zeros((3, 9)), DEV, cfgs, 4)
    with pytest.raises(_capi.EdmpError, match="n_obstacles"):
        IntersectionVolumeGuide(scenes.random_scene(0, 65), DEV, cfgs, 4)
    guide = IntersectionVolumeGuide(scenes.random_scene(0, 4), DEV, cfgs, 4)
    with pytest.raises(ValueError):
        guide.cost(torch.zeros(3, 7, 48), 10)  # t != 0 needs the full batch (per-row schedules)
    with pytest.raises(ValueError):
        guide.cost(torch.zeros(4, 6, 48), 0)
    dif = Diffusion(T, DEV)
    with pytest.raises(ValueError):
        dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=3, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL)
    with pytest.raises(ValueError):
        dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=4, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL,
                           noise=np.zeros((T + 1, 4, 7, 49)))
    bad_cfg = dict(cfgs)
    bad_cfg["guidance_method"] = np.array([0, 0.5, 1, 1.0])
    with pytest.raises(_capi.EdmpError, match="guidance_method"):
        IntersectionVolumeGuide(scenes.random_scene(0, 4), DEV, bad_cfg, 4)
    # the state is still usable after the failures
    X = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=4, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL, noise="device", seed=2, t_stop=T - 2)
    assert np.isfinite(X).all()


def _sharded_worker(rank, world, port, q):
    import os

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    from edmp_amd import dist as ED
    from edmp_amd import scenes
    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.temporalunet import TemporalUNet

    guides, bpg = [1, 11, 18, 10], 3  # grad_norm rows (11, 18) make the cross-rank norm matter
    cfgs = cfgs_for(guides, bpg)
    Btot = cfgs["total_batch_size"]
    lo, hi = ED.shard_rows(Btot, rank, world)
    sh = ED.shard_guide_cfgs(cfgs, lo, hi)
    net = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=W.init_state_dict(5, 7, 32, TINY_DIMS), max_batch=Btot)
    scene = scenes.random_scene(7, 8)
    guide = IntersectionVolumeGuide(scene, DEV, sh, hi - lo)
    dif = Diffusion(T, DEV)
    noise = noise_for(41, Btot)
    X = dif.denoise_guided(net, guide, 50, 7, sh["guidance_schedule"], batch_size=hi - lo, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL,
                           noise=np.ascontiguousarray(noise[:, lo:hi]), t_stop=T - 10, zero_row0=(rank == 0), allreduce=ED.allreduce_sum_)
    vols, idx = guide.row_swept_volumes(scenes.DEFAULT_START, scenes.DEFAULT_GOAL, X)
    best = ED.gather_best(float(vols[idx]), idx, X[idx], True)
    q.put((rank, lo, hi, X, best["rank"], best["index"], best["volume"]))
    dist.destroy_process_group()


def test_one_logical_batch_sharded_over_two_ranks():
    """BASELINE config 5 semantics: two processes each hold half the rows of ONE reference batch that has
    grad_norm rows; with the per-guided-step all-reduce of sum(g^2) the shards reproduce the single-process run, and the
    end-of-sampling gather picks the same row.  (gloo; both ranks share this box's GPU.)"""
    import socket

    import torch.multiprocessing as mp

    from edmp_amd import scenes
    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.temporalunet import TemporalUNet

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    out = sorted((q.get(timeout=300) for _ in range(2)), key=lambda o: o[0])
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    cfgs = cfgs_for([1, 11, 18, 10], 3)
    B = cfgs["total_batch_size"]
    net = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=W.init_state_dict(5, 7, 32, TINY_DIMS), max_batch=B)
    guide = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    Xref = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL,
                              noise=noise_for(41, B), t_stop=T - 10)
    Xsh = np.concatenate([out[0][3], out[1][3]], axis=0)
    assert (out[0][1], out[0][2], out[1][1], out[1][2]) == (0, 6, 6, 12)
    assert maxabs(Xsh, Xref) <= 1e-9, maxabs(Xsh, Xref)  # only the f64 summation order of sum(g^2) differs
    vols, idx = guide.row_swept_volumes(scenes.DEFAULT_START, scenes.DEFAULT_GOAL, Xref)
    owner, local = (0, idx) if idx < 6 else (1, idx - 6)
    assert out[0][4] == out[1][4] == owner and out[0][5] == out[1][5] == local
    # without the all-reduce the grad_norm rows would differ: the coupling is real
    g2 = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, {k: (v[:6] if hasattr(v, "shape") and v.shape[:1] == (12,) else v) for k, v in cfgs.items()}, 6)
    Xno = dif.denoise_guided(net, g2, 50, 7, cfgs["guidance_schedule"][:6], batch_size=6, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL,
                             noise=np.ascontiguousarray(noise_for(41, B)[:, :6]), t_stop=T - 10)
    assert maxabs(Xno, Xref[:6]) > 1e-6


def _nccl_worker(rank, world, port, q):
    import ctypes as C
    import functools
    import os

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist

    try:
        # one GPU per rank when the box has them (rank -> cuda:rank); on a one-GPU box every rank lands on cuda:0
        DEV = f"cuda:{rank % max(torch.cuda.device_count(), 1)}"  # noqa: N806 - shadows the module constant for this worker
        torch.cuda.set_device(torch.device(DEV))
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(DEV))
        from edmp_amd import dist as ED
        from edmp_amd import scenes
        from edmp_amd import weights as W
        from edmp_amd.diffusion import Diffusion
        from edmp_amd.guide import IntersectionVolumeGuide
        from edmp_amd.temporalunet import TemporalUNet

        # device-tensor collectives of the data path: scalar all-reduce, end-of-sampling all-gather + broadcast
        x = torch.full((1,), 2.5 + rank, dtype=torch.float64, device=DEV)
        ED.allreduce_sum_(x, always=True)
        torch.cuda.synchronize()
        traj = np.full((7, 50), float(rank))
        best = ED.gather_best(3.0 - rank, 5 + rank, traj, True, device=DEV, always=True)
        # the sharded reverse loop with the RCCL all-reduce enqueued from inside the device-resident loop
        cfgs = cfgs_for([1, 11, 18, 10], 3)
        Btot = cfgs["total_batch_size"]
        lo, hi = ED.shard_rows(Btot, rank, world)
        sh = ED.shard_guide_cfgs(cfgs, lo, hi)
        net = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=W.init_state_dict(5, 7, 32, TINY_DIMS), max_batch=Btot)
        guide = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, sh, hi - lo)
        dif = Diffusion(T, DEV)
        noise = np.ascontiguousarray(noise_for(41, Btot)[:, lo:hi])
        X = dif.denoise_guided(net, guide, 50, 7, sh["guidance_schedule"], batch_size=hi - lo, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL,
                               noise=noise, t_stop=T - 10, zero_row0=(rank == 0), allreduce=functools.partial(ED.allreduce_sum_, always=True))
        # the same run with the NATIVE hook (csrc/rccl_hook.hip: ncclAllReduce called by the device loop itself, own communicator from a
        # unique id broadcast over the process group), with torch's communicator borrowed, and under whole-run hipGraph replay
        kw = dict(batch_size=hi - lo, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL, noise=noise, t_stop=T - 10, zero_row0=(rank == 0))
        py_stats = dict(dif.hook_stats)
        hook = ED.RcclAllReduce(dif)
        Xn = dif.denoise_guided(net, guide, 50, 7, sh["guidance_schedule"], allreduce=hook, **kw)
        extra = {"python": py_stats, "native": dict(dif.hook_stats), "native_world": (hook.world, hook.rank, hook.kind), "X_native": Xn}
        # the hook is off outside its own runs: an unsharded run of the same context must not issue the collective
        dif.denoise_guided(net, guide, 50, 7, sh["guidance_schedule"], **kw)
        raw = (C.c_uint64 * 3)()
        dif.ctx.lib.edmp_sampler_allreduce_stats(dif.ctx.h, raw, 1)
        extra["calls_of_an_unsharded_run"] = int(raw[0])
        dif.ctx.lib.edmp_sampler_set_graph(dif.ctx.h, 1)
        noise_dev = dif.ctx.to_dev(noise, torch.float64)  # (graph replay keys on the resident noise pointer)
        kw["noise"] = noise_dev
        Xg = [dif.denoise_guided(net, guide, 50, 7, sh["guidance_schedule"], allreduce=hook, **kw) for _ in range(3)]
        dif.ctx.lib.edmp_sampler_set_graph(dif.ctx.h, 0)
        extra["X_graph"] = Xg[-1]
        kw["noise"] = noise
        hook.close()
        try:
            comm = dist.distributed_c10d._get_default_group()._get_backend(torch.device(DEV))._comm_ptr()
            hb = ED.RcclAllReduce(dif, comm_ptr=comm)
            extra["X_borrowed"] = dif.denoise_guided(net, guide, 50, 7, sh["guidance_schedule"], allreduce=hb, **kw)
            extra["borrowed_world"] = (hb.world, hb.rank, hb.kind)
            hb.close()
        except AttributeError as exc:  # a torch without ProcessGroupNCCL._comm_ptr
            extra["borrowed_skipped"] = repr(exc)
        q.put(("ok", rank, float(x.item()), best["rank"], best["index"], best["volume"], float(best["traj"][0, 0]), lo, hi, extra, X))
        dist.destroy_process_group()
    except Exception as exc:  # reported to the parent: a second rank on the same GPU is refused by RCCL
        q.put(("error", rank, repr(exc)))


def _spawn(target, world, timeout=300):
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    out = []
    try:
        for _ in range(world):
            out.append(q.get(timeout=timeout))
    finally:
        for p in ps:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    return sorted(out, key=lambda o: o[1])


def test_rccl_branch_world_size_one():
    """The `nccl` (= RCCL) branch of edmp_amd.dist on the one GPU a test box has: process group of ONE rank, device
    tensors, the collectives actually issued (always=True): scalar all-reduce, all-gather + broadcast of the best
    trajectory, and the per-guided-step all-reduce called from inside the device-resident loop through
    edmp_sampler_set_allreduce - the result must equal the plain single-process run bit for bit."""
    from edmp_amd import scenes
    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.temporalunet import TemporalUNet

    out = _spawn(_nccl_worker, 1)
    assert out[0][0] == "ok", out[0]
    _, rank, x, brank, bidx, bvol, t00, lo, hi, extra, X = out[0]
    assert x == 2.5 and (brank, bidx, bvol, t00) == (0, 5, 3.0, 0.0)
    # the native hook: same result bit for bit, one call per guided step (t = 255..246: 5 even steps), off outside its runs
    assert np.array_equal(extra["X_native"], X) and np.array_equal(extra["X_graph"], X)
    assert extra["native_world"] == (1, 0, "own communicator") and extra["native"]["calls"] == extra["python"]["calls"] == 5
    assert extra["native"]["kind"].startswith("native") and extra["python"]["kind"].startswith("python")
    assert extra["calls_of_an_unsharded_run"] == 0
    if "X_borrowed" in extra:
        assert np.array_equal(extra["X_borrowed"], X) and extra["borrowed_world"] == (1, 0, "borrowed communicator")
    print(f"hook host time per call: python {1e6 * extra['python']['total_s'] / 5:.1f} us, native {1e6 * extra['native']['total_s'] / 5:.1f} us")
    cfgs = cfgs_for([1, 11, 18, 10], 3)
    B = cfgs["total_batch_size"]
    assert (lo, hi) == (0, B)
    net = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=W.init_state_dict(5, 7, 32, TINY_DIMS), max_batch=B)
    guide = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, B)
    Xref = Diffusion(T, DEV).denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL,
                                            noise=noise_for(41, B), t_stop=T - 10)
    assert np.array_equal(X, Xref)


def test_rccl_two_ranks():
    """Two RCCL ranks, the sharded loop over a real all-reduce.  With >= 2 GPUs visible each rank takes its own device
    (rank -> cuda:rank, xGMI between them) and the result must equal the single-process run of the whole batch to 1e-9
    (only the f64 summation order of sum(g^2) differs).  RCCL refuses two ranks on one device: with fewer than two GPUs the
    test skips before starting any rank."""
    from edmp_amd import scenes
    from edmp_amd import weights as W
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.temporalunet import TemporalUNet

    ngpu = torch.cuda.device_count()
    if ngpu < 2:  # RCCL refuses two ranks on one device
        pytest.skip(f"needs 2 GPUs, found {ngpu}")
    out = _spawn(_nccl_worker, 2, timeout=300)
    errs = [o for o in out if o[0] == "error"]
    assert not errs, errs
    cfgs = cfgs_for([1, 11, 18, 10], 3)
    B = cfgs["total_batch_size"]
    assert [o[0] for o in out] == ["ok", "ok"] and out[0][2] == out[1][2] == 6.0  # 2.5 + 3.5
    assert (out[0][3], out[0][4], out[0][5], out[0][6]) == (out[1][3], out[1][4], out[1][5], out[1][6]) == (1, 6, 2.0, 1.0)  # rank 1 holds the smaller volume
    Xsh = np.concatenate([out[0][-1], out[1][-1]])
    for key in ("X_native", "X_graph", "X_borrowed"):  # the native hook sums the same two f64 partials: identical to the Python hook's run
        if key in out[0][9]:
            assert np.array_equal(np.concatenate([out[0][9][key], out[1][9][key]]), Xsh), key
    assert out[0][9]["native_world"] == (2, 0, "own communicator") and out[1][9]["native_world"] == (2, 1, "own communicator")
    assert Xsh.shape[0] == B and (out[0][7], out[0][8], out[1][7], out[1][8]) == (0, B // 2, B // 2, B)
    net = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=W.init_state_dict(5, 7, 32, TINY_DIMS), max_batch=B)
    guide = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, B)
    Xref = Diffusion(T, DEV).denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], batch_size=B, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL,
                                            noise=noise_for(41, B), t_stop=T - 10)
    assert maxabs(Xsh, Xref) <= 1e-9, maxabs(Xsh, Xref)


def _run_bench_under_torchrun(extra, nproc=2, timeout=900):
    """bench.py launched exactly as the driver's scaling run does (python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...); on a box with fewer GPUs than
    ranks the ranks share the device over gloo (EDMP_DIST_BACKEND=gloo), with enough GPUs the real RCCL path runs."""
    import json
    import os
    import socket
    import subprocess
    import sys

    from tests.conftest import ROOT

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if torch.cuda.device_count() < nproc:
        env["EDMP_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-roofline", *extra]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 prints exactly one JSON line
    return json.loads(lines[0])


@pytest.mark.parametrize("mode", ["replicas", "logical_batch"])
def test_bench_two_ranks_under_torchrun(mode):
    """the driver's N > 1 launch path of bench.py (BASELINE configs 4 and 5; reference: one process per device,
    /root/reference/benchmark/cfgs/cfg2.yaml:2,14): plain row-sharded replicas with the end-of-sampling gather, and one
    logical batch of 2048 rows over the 8-guide ensemble with the per-guided-step all-reduce inside the device loop."""
    import math

    extra = [] if mode == "replicas" else ["--logical-batch", "--guides", "1,2,3,4,5,10,11,13"]
    d = _run_bench_under_torchrun(extra)
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 2048 and d["steps"] == 1 and d["scaling"] == "weak"
    assert math.isfinite(d["value"]) and d["value"] > 0 and abs(d["value"] - 2048 * 255 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    sp = d["success_proxy"]
    assert sp["rows"] == 2048 and 0 <= sp["rows_ok"] <= sp["rows_collision_free"] <= 2048 and sp["collision_free_rate"] == sp["rows_collision_free"] / 2048
    assert d["n_ranks_seen"] == 2
    assert ("logical batch" in d["config"]["parallelism"]) == (mode == "logical_batch")


def test_bench_plain_launch_with_gpus_2_spawns_two_ranks():
    """`python bench.py --gpus 2` started WITHOUT torch.distributed.run must not fall through to one rank and
    print a mislabelled line: it runs itself under the launcher in a child process (gloo over the one GPU of a test box, RCCL with two) and the
    line reports the world size the process group summed (`n_ranks_seen`).  With too few GPUs and the RCCL backend it refuses."""
    import json
    import os
    import subprocess
    import sys

    from tests.conftest import ROOT

    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    few = torch.cuda.device_count() < 2
    if few:
        refuse = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-roofline"],
                                cwd=ROOT, env={**env, "EDMP_DIST_BACKEND": "nccl"}, capture_output=True, text=True, timeout=300)
        assert refuse.returncode != 0 and "GPU(s) visible" in refuse.stderr and not [l for l in refuse.stdout.splitlines() if l.startswith("{")]
        env["EDMP_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-roofline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["n_ranks_seen"] == 2 and d["config"]["global_batch"] == 2048
    assert d["dist_backend"] == ("gloo" if few else "nccl")


def test_eight_ranks_shake_out_on_this_box(tmp_path):
    """the driver's N = 8 launch, before the first 8-GPU lease - `python bench.py --gpus 8` (run under the
    launcher in a child process) and `torch.distributed.run --nproc-per-node 8 infer_serial.py --max-scenes 16` with EIGHT processes (RCCL, one rank per
    GPU): ports, rendezvous, per-rank memory, the summed world size and the scene deal.  Reference launch model: one process per
    device (benchmark/cfgs/cfg2.yaml:2,14).  With fewer than eight GPUs it skips before starting any rank: eight ranks sharing one
    device would hold it from ten processes at once (pytest and the launching bench.py included)."""
    import json
    import os
    import socket
    import subprocess
    import sys

    import yaml

    from tests.conftest import ROOT

    ngpu = torch.cuda.device_count()
    if ngpu < 8:
        pytest.skip(f"needs 8 GPUs, found {ngpu}")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--batch", "64", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-roofline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["n_ranks_seen"] == 8 and d["config"]["global_batch"] == 512 and d["success_proxy"]["rows"] == 512
    assert d["dist_backend"] == "nccl" and np.isfinite(d["value"]) and d["value"] > 0
    assert 0 <= d["best"]["rank"] < 8

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cfg_c1_plumbing.yaml")))
    cfg["dataset"]["scene_types"] = ["tabletop", "stress"]
    cfg["dataset"]["num_scenes_per_type"] = 9  # 18 scenes in the cfg, --max-scenes stops at 16
    os.makedirs(tmp_path / "cfgs")
    cj = tmp_path / "cfgs" / "cfg_eighteen_scenes.yaml"
    yaml.safe_dump(cfg, open(cj, "w"))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = tmp_path / "res.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "infer_serial.py"), "-c", str(cj), "--seed", "3", "--max-scenes", "16", "--results-json", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    sm = json.load(open(out))["summary"]
    rows_per_scene = cfg["guide"]["batch_size_per_guide"] * len(cfg["guide"]["guides"])
    assert sm["ranks"] == 8 and sm["scenes"] == 16 and sm["scenes_per_rank"] == [2] * 8 and sm["rows"] == 16 * rows_per_scene
    for rk in range(1, 8):
        dk = json.load(open(str(out) + f".rank{rk}"))
        assert dk["summary"] == sm and len(dk["scenes"]) == 2
    assert "16 scenes on 8 rank(s)" in r.stdout


def test_allreduce_hook_inside_the_device_loop(tiny_net):
    """edmp_sampler_set_allreduce: the hook is called once per guided step with the context's stream and the device
    scalar; an identity hook leaves the run bit-identical, a hook that doubles sum(g^2) changes exactly the grad_norm rows."""
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide

    net, _ = tiny_net
    cfgs = cfgs_for([1, 11], 2)
    B = cfgs["total_batch_size"]
    guide = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, B)
    dif = Diffusion(T, DEV)
    noise = noise_for(5, B)
    kw = dict(batch_size=B, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL, noise=noise, t_stop=T - 12)
    Xref = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], **kw)
    calls = []

    def ident(t):
        calls.append(int(t.numel()))
        return t

    X1 = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], allreduce=ident, **kw)
    assert np.array_equal(X1, Xref) and len(calls) == 6 and set(calls) == {1}  # t = 254, 252, ..., 244

    def double(t):
        t.mul_(2.0)
        return t

    X2 = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], allreduce=double, **kw)
    gn = np.asarray(cfgs["grad_norm"]) > 0
    assert np.array_equal(X2[~gn], Xref[~gn]) and not np.array_equal(X2[gn], Xref[gn])

    def boom(t):
        raise RuntimeError("collective failed")

    with pytest.raises(RuntimeError, match="collective failed"):
        dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], allreduce=boom, **kw)
    assert np.array_equal(dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], **kw), Xref)  # hook removed, state usable


def test_best_trajectory_nan_semantics():
    """torch.argmin (lib/guide.py:650) treats NaN as the smallest value: the first NaN row wins; edmp's argmin kernel and
    the cross-rank gather follow it."""
    from edmp_amd import _capi
    from edmp_amd.runtime import get_context, ptr

    ctx = get_context(DEV)
    lib = ctx.lib
    for vals, want in (([3.0, 1.0, 2.0, 1.0], 1), ([3.0, float("nan"), 0.5, float("nan")], 1), ([float("nan")] * 3, 0), ([float("inf"), 5.0], 1)):
        v = ctx.to_dev(np.asarray(vals, dtype=np.float32), torch.float32)
        out = C_int()
        _capi.check(lib.edmp_argmin_dev(ctx.h, ptr(v), len(vals), byref(out)))
        ctx.sync()
        assert out.value == want == int(torch.argmin(torch.tensor(vals)))


def test_reference_written_checkpoint_on_the_gpu():
    """G14: the checkpoint directory written by the reference's TemporalUNet.save() loads through
    TemporalUNet(model_name=<dir>) exactly like the reference's load() (temporalunet.py:88-92) and the HIP forward
    reproduces the reference's own output."""
    import os

    from edmp_amd.temporalunet import TemporalUNet

    d = os.path.join(os.path.dirname(__file__), "golden", "g14_ref_checkpoint")
    fw = np.load(os.path.join(d, "forward.npz"))
    net = TemporalUNet(d, 7, 32, DEV, dims=tuple(int(v) for v in fw["dims"]), max_batch=4)
    y = net(torch.tensor(fw["x"]), torch.tensor(fw["t"])).cpu().numpy()
    assert np.abs(y - fw["y"]).max() <= 2e-5, np.abs(y - fw["y"]).max()


def test_resident_slots_keep_alternating_objects_loaded(tiny_net):
    """A context keeps several models and guides resident (edmp_unet_slot / edmp_guide_slot): alternating between two
    TemporalUNets and between per-scene guides re-uploads nothing, and results are those of freshly bound objects."""
    from edmp_amd import _capi, scenes
    from edmp_amd import weights as W
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import get_context
    from edmp_amd.temporalunet import TemporalUNet

    ctx = get_context(DEV)
    net_a, _ = tiny_net
    net_b = TemporalUNet(None, 7, 32, DEV, dims=TINY_DIMS, state_dict=W.init_state_dict(6, 7, 32, TINY_DIMS), max_batch=8)
    x = torch.randn(3, 7, 50, generator=torch.Generator().manual_seed(1))
    t = torch.tensor([40.0])
    ya, yb = net_a(x, t).cpu().numpy(), net_b(x, t).cpu().numpy()
    assert not np.array_equal(ya, yb)
    loads = []
    orig = ctx.lib.edmp_unet_load

    def counting(*a):
        loads.append(1)
        return orig(*a)

    ctx.lib.edmp_unet_load = counting
    try:
        for _ in range(3):
            assert np.array_equal(net_a(x, t).cpu().numpy(), ya) and np.array_equal(net_b(x, t).cpu().numpy(), yb)
    finally:
        ctx.lib.edmp_unet_load = orig
    assert not loads, "alternating between two resident models must not re-upload weights"
    cfgs = cfgs_for([1, 10], 2)
    guides = [IntersectionVolumeGuide(scenes.random_scene(s, 5), DEV, cfgs, 4) for s in (1, 2, 3)]
    q = torch.tensor(np.random.RandomState(0).uniform(-1, 1, (4, 7, 48)))
    ref = [g.cost(q, 0).cpu().numpy() for g in guides]
    sets = []
    orig_s = ctx.lib.edmp_scene_set

    def counting_s(*a):
        sets.append(1)
        return orig_s(*a)

    ctx.lib.edmp_scene_set = counting_s
    try:
        for _ in range(2):
            for g, r in zip(guides, ref):
                assert np.array_equal(g.cost(q, 0).cpu().numpy(), r)
    finally:
        ctx.lib.edmp_scene_set = orig_s
    assert not sets, "switching between resident per-scene guides must not rebuild the obstacle table"
    # beyond the capacity (8 guides per context) the least recently used slot is evicted and transparently rebuilt
    many = [IntersectionVolumeGuide(scenes.random_scene(10 + s, 3), DEV, cfgs, 4) for s in range(9)]
    assert np.array_equal(guides[0].cost(q, 0).cpu().numpy(), ref[0]) and tuple(many[0].cost(q, 0).shape) == (4, 48, 9 * 3)


def test_packed_weight_image_round_trip(tmp_path, monkeypatch):
    """TemporalUNet.pack(): the device weight image written next to the checkpoint loads with one mmap + one copy and
    gives bit-identical outputs; a stale image (older than the checkpoint, other architecture, other builder switches) is
    ignored."""
    import os
    import time as _time

    from edmp_amd import weights as W
    from edmp_amd.temporalunet import TemporalUNet

    d = str(tmp_path / "TemporalUNetModel255_N50")
    sd = W.init_state_dict(9, 7, 32, FULL_DIMS)
    W.save_checkpoint_dir(d, sd)
    x = torch.randn(5, 7, 50, generator=torch.Generator().manual_seed(2))
    t = torch.tensor([31.0])
    t0 = _time.perf_counter()
    a = TemporalUNet(d, 7, 32, DEV, dims=FULL_DIMS, max_batch=8)
    t_sd = _time.perf_counter() - t0
    ya = a(x, t).cpu().numpy()
    path = a.pack()
    assert os.path.basename(path) == W.PACKED_NAME and os.path.getsize(path) > 80e6  # < 120 MB: taps that only ever meet zero padding (L = 2) are not stored
    t0 = _time.perf_counter()
    b = TemporalUNet(d, 7, 32, DEV, dims=FULL_DIMS, max_batch=8)
    t_pk = _time.perf_counter() - t0
    assert b._packed is not None and b._flat is None
    assert np.array_equal(b(x, t).cpu().numpy(), ya)
    print(f"load from state dict {t_sd:.2f} s, from the packed image {t_pk:.2f} s")
    # builder switches that move tensors inside the image WITHOUT changing its size: the layout id covers the
    # layout actually produced, so the image is refused and the state dict is loaded instead - same network, other kernels
    for env in ("EDMP_NO_RESFOLD", "EDMP_NO_KARATSUBA", "EDMP_NO_LEVEL", "EDMP_BF16X3"):
        monkeypatch.setenv(env, "0" if env == "EDMP_BF16X3" else "1")
        e = TemporalUNet(d, 7, 32, DEV, dims=FULL_DIMS, max_batch=8)
        monkeypatch.delenv(env)
        assert e._packed is None and e._flat is not None, env
        ye = e(x, t).cpu().numpy()
        assert rmse(ye, ya) <= 1e-5 and not np.array_equal(ye, ya), env
        lay = C_int()
        e.ctx.lib.edmp_unet_packed_size(e.ctx.h, byref(lay))
        assert lay.value != b._packed["layout"], env
    # another architecture in the same directory: the image is ignored, the state dict decides (and fails on shapes)
    with pytest.raises((ValueError, KeyError)):
        TemporalUNet(d, 7, 32, DEV, dims=TINY_DIMS, max_batch=8)
    # a newer checkpoint invalidates the image
    sd2 = W.init_state_dict(10, 7, 32, FULL_DIMS)
    _time.sleep(1.1)
    W.save_checkpoint_dir(d, sd2)
    c = TemporalUNet(d, 7, 32, DEV, dims=FULL_DIMS, max_batch=8)
    assert c._packed is None and not np.array_equal(c(x, t).cpu().numpy(), ya)
    b.save()  # a model constructed from the image can still write the reference's state-dict format


def _adversarial_state_dict(kind, seed):
    """the seeded full-size weights with the k5 Conv1dBlock filters (blocks.py:13-34) reshaped into cases that stress the
    Karatsuba forms w2 (x0 + x1) + (w3 - w2) x1 of the L = 2 / L = 4 levels (wide.hip): their rounding error scales with
    |w2| |x|, not with the result."""
    from edmp_amd import weights as W

    sd = W.init_state_dict(seed, 7, 32, FULL_DIMS)
    rs = np.random.RandomState(seed + 100)
    for name, w in sd.items():
        if not (name.endswith(".block.0.weight") and w.ndim == 3 and w.shape[2] == 5):
            continue
        w = w.astype(np.float64)
        if kind == "centre":      # a trained smoothing filter: centre tap dominant
            w[:, :, 2] *= 30.0
        elif kind == "heavy":     # heavy-tailed taps (Student t, 2 degrees of freedom)
            w *= np.clip(np.abs(rs.standard_t(2, w.shape)), 0.05, 50.0)
        elif kind == "equal":     # w1 ~ w2 ~ w3: the differences w3 - w2, w1 - w2 cancel catastrophically
            for k in (1, 3):
                w[:, :, k] = w[:, :, 2] * (1.0 + 1e-4 * rs.standard_normal(w.shape[:2]))
        elif kind == "scale":     # per-output-channel scale spread 1e-3 .. 1e3
            w *= (10.0 ** rs.uniform(-3, 3, (w.shape[0], 1, 1)))
        else:
            raise ValueError(kind)
        sd[name] = w.astype(np.float32)
    return sd


@pytest.mark.parametrize("kind", ["centre", "heavy", "equal", "scale"])
def test_karatsuba_forms_with_adversarial_weights(oracle, monkeypatch, kind):
    """Full-size forward vs the oracle with weight distributions that are hostile to the bilinear (Karatsuba) forms, at the
    UNCHANGED gates of the random-init test (rmse 2e-5, max 2e-4); the error of the Karatsuba build, of the direct-form
    build (EDMP_NO_KARATSUBA=1) and of torch's own float32 forward are measured against a float64 evaluation of the same
    network and printed.  Conv1dBlock: /root/reference/diffusion/models/blocks.py:13-34."""
    from edmp_amd.temporalunet import TemporalUNet

    sd = _adversarial_state_dict(kind, 31)
    B = 37
    x = torch.tensor(np.random.RandomState(6).standard_normal((B, 7, 50)) * 1.5, dtype=torch.float32)
    t = torch.tensor([123.0])
    with torch.no_grad():
        ref32 = oracle.unet_forward({k: torch.from_numpy(v) for k, v in sd.items()}, x, t).numpy()
        ref64 = oracle.unet_forward({k: torch.from_numpy(v).double() for k, v in sd.items()}, x.double(), t.double()).numpy()
    kar = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=B)(x, t).cpu().numpy()
    monkeypatch.setenv("EDMP_NO_KARATSUBA", "1")
    direct = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=B)(x, t).cpu().numpy()
    monkeypatch.delenv("EDMP_NO_KARATSUBA")
    e_k, e_d, e_t = rmse(kar, ref64), rmse(direct, ref64), rmse(ref32, ref64)
    print(f"\n[karatsuba/{kind}] rms(eps) {float(np.sqrt(np.mean(ref64 ** 2))):.3g}; rmse vs f64: karatsuba {e_k:.3e}, direct {e_d:.3e}, torch f32 {e_t:.3e}; "
          f"ratio karatsuba/direct {e_k / max(e_d, 1e-30):.2f}; vs the f32 oracle: rmse {rmse(kar, ref32):.3e} max {maxabs(kar, ref32):.3e}")
    assert not np.array_equal(kar, direct)  # the switch really selects another kernel form
    assert rmse(kar, ref32) <= 2e-5 and maxabs(kar, ref32) <= 2e-4, (kind, rmse(kar, ref32), maxabs(kar, ref32))
    assert rmse(direct, ref32) <= 2e-5 and maxabs(direct, ref32) <= 2e-4, (kind, rmse(direct, ref32), maxabs(direct, ref32))
    assert e_k <= 3.0 * max(e_d, e_t), (kind, e_k, e_d, e_t)


@pytest.mark.parametrize("kind", ["centre", "heavy", "equal", "scale"])
def test_bf16x3_split_layers_are_at_least_as_accurate_as_the_fp32_mfma_layers(oracle, monkeypatch, kind):
    """Round 6 (csrc/bf3.hip): the Conv1dBlocks at L = 13 / L = 7 / L = 4 and the six resampling convs of the >= 128-channel levels run on the bf16
    matrix pipe as six EXACT bf16 x bf16 partial products per fp32 product with fp32 accumulation.  The adoption bar: on the
    four hostile weight families the error against a float64 evaluation of the same network must not exceed 1.25 x the fp32-MFMA build's
    (EDMP_BF16X3=0) - rmse on eps and on the activations behind the affected levels (down2: everything upstream is the same kernels in
    both builds, so the difference IS the layers); the max over a few thousand elements is an extreme-value statistic (+-15 % between
    two correct kernels), held to 1.5 x here - and every gate against the f32 oracle is unchanged.  The per-INSTANCE criterion (same inputs
    to both kernels, 6 x L x C float64 outputs, rmse AND max <= 1.25 x; measured x0.43-0.62 / x0.36-0.89) is tools/bf3bench6.hip,
    profiles/r06_bf16x3.md.  Conv1dBlock: /root/reference/diffusion/models/blocks.py:13-34; resamplers :213, :251."""
    from edmp_amd.temporalunet import TemporalUNet

    sd = _adversarial_state_dict(kind, 31)
    B = 37
    x = torch.tensor(np.random.RandomState(6).standard_normal((B, 7, 50)) * 1.5, dtype=torch.float32)
    t = torch.tensor([123.0])
    tr64, tr32 = {}, {}
    with torch.no_grad():
        ref32 = oracle.unet_forward({k: torch.from_numpy(v) for k, v in sd.items()}, x, t, trace=tr32).numpy()
        ref64 = oracle.unet_forward({k: torch.from_numpy(v).double() for k, v in sd.items()}, x.double(), t.double(), trace=tr64).numpy()
    taps = {"down2": 2, "down3": 3, "down4": 4, "up1": 201, "up2": 202}

    def run(mask):
        if mask is not None:
            monkeypatch.setenv("EDMP_BF16X3", mask)
        net = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, state_dict=sd, max_batch=B)
        monkeypatch.delenv("EDMP_BF16X3", raising=False)
        y = net(x, t).cpu().numpy()
        acts = {k: net.activation(w, B).cpu().numpy() for k, w in taps.items()}
        names = {n for n, _, _, _ in net.ctx.prof_ops()}
        return y, acts, names, net.flops_by_pipe()

    y_n, a_n, names_n, pipes_n = run("0")
    y_s, a_s, names_s, pipes_s = run(None)
    assert not any(n.startswith("bf3_") for n in names_n) and pipes_n[1] == 0.0
    assert {"bf3_conv_kernel<0, 32, 32, 32, 7, false>", "bf3_conv_kernel<0, 32, 32, 32, 7, true>", "bf3_conv_kernel<0, 16, 32, 16, 7, false>", "bf3_conv_kernel<0, 16, 32, 16, 7, true>",
            "bf3_conv_kernel<0, 16, 32, 16, 13, false>", "bf3_conv_kernel<0, 16, 32, 16, 13, true>", "bf3_conv_kernel<1, 32, 32, 32, 7, false>", "bf3_conv_kernel<2, 32, 32, 32, 4, false>",
            "bf3_conv_kernel<1, 32, 32, 32, 4, false>", "bf3_conv_kernel<2, 32, 32, 32, 2, false>", "bf3_conv_kernel<1, 16, 32, 16, 13, false>", "bf3_conv_kernel<2, 16, 32, 16, 7, false>",
            "bf3_conv_kernel<0, 32, 64, 64, 4, false>", "bf3_conv_kernel<0, 32, 64, 64, 4, true>", "bf3_conv_kernel<0, 32, 32, 32, 4, false>", "bf3_conv_kernel<0, 32, 32, 32, 4, true>"} <= names_s
    assert pipes_s[1] > 0 and pipes_s[0] < pipes_n[0]
    assert not np.array_equal(y_n, y_s)
    rows = [("eps", y_n, y_s, ref64)] + [(k, a_n[k], a_s[k], tr64[k].numpy()) for k in taps]
    for name, n_, s_, r_ in rows:
        en, es, mn, ms_ = rmse(n_, r_), rmse(s_, r_), maxabs(n_, r_), maxabs(s_, r_)
        print(f"\n[bf16x3/{kind}] {name}: rms {float(np.sqrt(np.mean(r_ ** 2))):.3g}; vs f64 rmse native {en:.3e} split {es:.3e} (x{es / en:.2f}); max native {mn:.3e} split {ms_:.3e} (x{ms_ / mn:.2f})")
        assert es <= 1.25 * en, (kind, name, es, en)
        assert ms_ <= 1.5 * mn, (kind, name, ms_, mn)
    assert rmse(y_s, ref32) <= 2e-5 and maxabs(y_s, ref32) <= 2e-4, (kind, rmse(y_s, ref32), maxabs(y_s, ref32))
    for k in taps:
        assert maxabs(a_s[k], tr32[k].numpy()) <= 5e-4 * max(1.0, float(np.abs(tr32[k].numpy()).max()) / 8), k


def test_kernels_of_other_streams_do_not_perturb_a_scene():
    """Round 6: two independent scenes on two contexts (streams, host threads) of one GPU - infer_serial's scenes in flight - must
    each reproduce their serial result bit for bit, repeatedly.  With the bf16x3 workgroups sharing CUs with other streams' kernels,
    ~5 % of such runs had ONE gradient element of one row changed (lanes 48-63 of a register of a co-resident guide wave;
    profiles/r06_coresidency_fault.md); the bf16x3 kernels now claim their waves' whole register budget, i.e. the CU."""
    import threading

    from edmp_amd import guide_cfg as GC
    from edmp_amd import scenes
    from edmp_amd.diffusion import Diffusion
    from edmp_amd.guide import IntersectionVolumeGuide
    from edmp_amd.runtime import get_context, lane_context
    from edmp_amd.temporalunet import TemporalUNet

    B, steps, reps = 1024, 2, 40
    guides = [1, 2, 3, 4, 5, 10]
    cfgs = GC.build_guide_cfgs([GC.catalog_guide_dict(g) for g in guides], 0, T, rows_per_guide=GC.split_rows(B, len(guides)))
    objs = []
    for lane in (0, 1):
        ctx = get_context(DEV) if lane == 0 else lane_context(0, 1)
        net = TemporalUNet(None, 7, 32, ctx, dims=FULL_DIMS, seed=1, max_batch=B)
        guide = IntersectionVolumeGuide(scenes.random_scene(11 + lane, 16), ctx, cfgs, B)
        dif = Diffusion(T, ctx)
        noise = ctx.to_dev(np.random.RandomState(99 + lane).standard_normal((T + 1, B, 7, 50)), torch.float64)
        kw = dict(batch_size=B, start=scenes.DEFAULT_START, goal=scenes.DEFAULT_GOAL, noise=noise, t_stop=T - steps)
        ref = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], **kw)
        objs.append((dif, net, guide, kw, ref))
    bad, errors = [[], []], []

    def work(lane):
        try:
            dif, net, guide, kw, ref = objs[lane]
            for rep in range(reps):
                X = dif.denoise_guided(net, guide, 50, 7, cfgs["guidance_schedule"], **kw)
                if not np.array_equal(X, ref):
                    bad[lane].append((rep, np.unique(np.nonzero(X != ref)[0])[:8].tolist()))
        except BaseException as exc:
            errors.append(exc)

    ths = [threading.Thread(target=work, args=(lane,)) for lane in (0, 1)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    if errors:
        raise errors[0]
    assert bad == [[], []], bad


def test_context_close_releases_the_gpu_and_lanes_are_cached():
    """secondary contexts (scenes in flight) used to leak a resident UNet + activation buffers + streams per
    infer_serial.run call.  Lanes are now cached per (device, lane) and an explicitly created Context can be closed."""
    from edmp_amd import _capi
    from edmp_amd.runtime import Context, lane_context
    from edmp_amd.temporalunet import TemporalUNet

    assert lane_context(DEV, 1) is lane_context(DEV, 1) and lane_context(DEV, 0) is not lane_context(DEV, 1)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    with Context(0) as ctx:
        net = TemporalUNet(None, 7, 32, ctx, dims=(32, 64, 128, 256, 512, 512), seed=3, max_batch=256)
        y = net(torch.randn(256, 7, 50, device=DEV), torch.tensor([7.0]))
        assert torch.isfinite(y).all()
        free1, _ = torch.cuda.mem_get_info()
        assert free0 - free1 > 90e6  # the 92 MB weight image + activations live in the context
        del y
    free2, _ = torch.cuda.mem_get_info()
    assert free0 - free2 < 0.25 * (free0 - free1), (free0, free1, free2)  # edmp_ctx_destroy gave the library's allocations back
    assert ctx.h is None
    ctx.close()  # idempotent
    with pytest.raises((_capi.EdmpError, Exception)):
        net(torch.randn(4, 7, 50, device=DEV), torch.tensor([7.0]))


def _independent_issued_flops(dims, horizon, cin0_stored, bf3_mask, karatsuba=True):
    """Issued matrix FLOPs per trajectory of every launch of the layer program, counted HERE from the architecture alone
    (/root/reference/diffusion/models/temporalunet.py:47-76, blocks.py:13-34,137-166,213,251) and the documented kernel forms - nothing is read
    from the library: per Conv1dBlock 2 x products x Cout x Cin_stored with products = the (output position, tap) pairs that meet a real input
    position (direct form; padding taps are never issued), 3 at L = 2 / 512 channels (Karatsuba), 9 at L = 4 / >= 256 channels (nested form,
    unless the bf16x3 mask moves that block to the direct form on the bf16 pipe); + 2 L Cout Cin for a folded residual 1x1 conv.
    Returns [(what, fp32-equivalent issued FLOPs, bf16-pipe FLOPs)] in program order; whole-level kernels (<= 64 channels) are one entry per level."""
    def pairs(Lin, Lout, k, stride, pad, tr):
        n = 0
        for lo in range(Lout):
            for tp in range(k):
                if not tr:
                    n += 0 <= lo * stride + tp - pad < Lin
                else:
                    q = lo + pad - tp
                    n += q >= 0 and q % stride == 0 and q // stride < Lin
        return n

    def bf3(cout, L, kind):
        cg, m = cout // 8, bf3_mask
        table = {"k5": {(32, 7): 1, (16, 7): 2, (16, 13): 4, (64, 4): 64, (32, 4): 128}, "down": {(32, 7): 8, (64, 4): 16, (16, 13): 32},
                 "up": {(32, 4): 8, (64, 2): 16, (16, 7): 32}}[kind]
        return bool(m & table.get((cg, L), 0))

    def block(cin, cout, L, res):  # one Conv1dBlock launch (+ folded residual 1x1 conv)
        direct = 2.0 * pairs(L, L, 5, 1, 2, False) * cout * cin
        on_bf16 = bf3(cout, L, "k5")
        if on_bf16 or not karatsuba:
            issued = direct
        elif L == 2 and cout // 8 == 64:
            issued = 2.0 * 3 * cout * cin
        elif L == 4 and cout // 8 >= 32:
            issued = 2.0 * 9 * cout * cin
        else:
            issued = direct
        r = 2.0 * L * cout * cin if res else 0.0
        return issued + r, (6.0 * (direct + r) if on_bf16 else 0.0)

    def up_len(L):
        return 2 * L - (1 if 2 * L in (8, 14, 26) else 0)  # the reference crops the up-sampled tensor to the skip's length

    out = []
    chans = [cin0_stored] + list(dims)
    L = horizon
    nd = len(dims)
    lens = []
    for i in range(nd):
        cin, c = chans[i], chans[i + 1]
        last = i == nd - 1
        lens.append(L)
        Lout = (L - 1) // 2 + 1
        if c <= 64 and not last:  # whole-level kernel: 2 residual blocks + k3s2
            f = sum(block(a, c, L, False)[0] for a in (cin, c, c, c)) + 2.0 * L * c * cin + 2.0 * pairs(L, Lout, 3, 2, 1, False) * c * c
            out.append((f"level down {cin}->{c} L={L}", f, 0.0))
        else:
            for a, res in ((cin, cin != c), (c, False), (c, False), (c, False)):
                out.append((f"block {a}->{c} L={L}", *block(a, c, L, res)))
            if not last:
                d = 2.0 * pairs(L, Lout, 3, 2, 1, False) * c * c
                out.append((f"k3s2 {c} L={L}", d, 6.0 * d if bf3(c, L, "down") else 0.0))
        if not last:
            L = Lout
    c = dims[-1]
    for a in (c, c, c, c):  # the two middle blocks
        out.append((f"mid block {c} L={L}", *block(a, c, L, False)))
    for i in range(nd - 1, 0, -1):  # (din, dout) = (dims[i-1], dims[i]): blocks 2*dout -> din, din -> din, ConvTranspose din
        din, dout = dims[i - 1], dims[i]
        Lo = up_len(L)
        final = i == 1
        if din <= 64:
            f = sum(block(a, din, L, False)[0] for a in (2 * dout, din, din, din)) + 2.0 * L * din * 2 * dout + 2.0 * pairs(L, Lo, 4, 2, 1, True) * din * din
            if final:
                f += block(din, din, Lo, False)[0]  # the final Conv1dBlock rides in the last level's launch
            out.append((f"level up {2 * dout}->{din} L={L}", f, 0.0))
        else:
            for a, res in ((2 * dout, True), (din, False), (din, False), (din, False)):
                out.append((f"block {a}->{din} L={L}", *block(a, din, L, res)))
            d = 2.0 * pairs(L, Lo, 4, 2, 1, True) * din * din
            out.append((f"convT {din} L={L}", d, 6.0 * d if bf3(din, L, "up") else 0.0))
        L = Lo
    return out


@pytest.mark.parametrize("mask", [0xff, 0x00])
def test_issued_flops_of_every_program_op_against_an_independent_count(mask, monkeypatch):
    """bench.py's roofline numerators come from the library under test (edmp_prof_ops / edmp_prof_ops_bf16).  Here every op's figure is
    recomputed from the architecture and the documented kernel forms alone and must agree exactly, for the default
    program (bf16x3 mask 0xff) and the all-fp32-MFMA program (mask 0)."""
    from edmp_amd.temporalunet import TemporalUNet

    monkeypatch.setenv("EDMP_BF16X3", hex(mask))
    net = TemporalUNet(None, 7, 32, DEV, dims=FULL_DIMS, seed=1, max_batch=8)
    net(torch.zeros(2, 7, 50), torch.tensor([3.0, 3.0]))  # binds the model: the context's program is this one
    ctx = net.ctx
    ops = [(nm, fl, fb) for (nm, _, _, fl), fb in zip(ctx.prof_ops(), ctx.prof_ops_bf16()) if fl > 0]
    levels = _independent_issued_flops(FULL_DIMS, 50, 8, mask)
    want, i = [], 0
    for nm, _, _ in ops:  # a merged level pair (level2_kernel: two levels per launch) is ONE op carrying both levels' work
        if i >= len(levels):
            break
        if nm.startswith("level2_kernel"):
            assert levels[i][0].startswith("level") and levels[i + 1][0].startswith("level"), (nm, levels[i][0], levels[i + 1][0])
            want.append((levels[i][0] + " + " + levels[i + 1][0], levels[i][1] + levels[i + 1][1], 0.0))
            i += 2
        else:
            want.append(levels[i])
            i += 1
    assert i == len(levels) and len(ops) == len(want), ([o[0] for o in ops], [w[0] for w in levels])
    for (nm, fl, fb), (what, f, b) in zip(ops, want):
        assert fl == f and fb == b, (nm, what, fl, f, fb, b)
    # totals: what bench.py divides by the measured time
    nominal, executed = net.flops_per_trajectory()
    f32, bf16 = net.flops_by_pipe()
    head = 2.0 * 50 * 7 * 32
    assert executed - head == sum(w[1] for w in want) and bf16 == sum(w[2] for w in want)
    assert f32 - head == sum(w[1] for w in want if w[2] == 0)
