"""State dicts that drive every GroupNorm -> Mish epilogue of the UNet out of the regime random initialisation keeps it in, and the
census that proves they do.  Shared by tests/test_hostile_weights_host.py (CPU: every Conv1dBlock of every architecture reaches the
regime, and the regime decides what it is meant to decide) and tests/test_gpu_hostile_activations.py (GPU: every epilogue copy against
the float64 oracle on these weights).  A plain module: no fixtures, no pytest hooks.

With weights.init_state_dict a GroupNorm input has group variances of 1e-2 and more, |mean| / std below 2, and a Mish input stays
inside -8 ... +6: the `+ 1e-5f` under the square root, the cancellation in x s + (beta - s mean) and the clamp at 20 of the fast Mish
never decide a result.  The four families change only what their regime needs, by a rule per Conv1dBlock (numbered in state-dict
order) and per GroupNorm group (the 8 contiguous channel blocks of a layer) - nothing is drawn, so every block of every
architecture gets there:

  offset    conv bias of group g += +-OFFSET (0.5 + g / 8), the sign alternating with g and with the block: |mean| >> std, the
            normalised value is the small difference of two large terms
  flat      conv weights and bias of group g scaled by 10^(-((g + block) mod 8) / 2): group variances from ~1e-1 down to ~1e-8,
            on both sides of eps = 1e-5, where eps and not the variance sets the scale
  dead      conv weights and bias of group (block mod 8) exactly zero: variance exactly 0, the output mish(beta) + addend, finite
            only through rstd = 1 / sqrt(0 + eps)
  saturate  GroupNorm gamma / beta by channel c mod 4: (SAT_GAIN, +SAT_BIAS), (-SAT_GAIN, -SAT_BIAS), (SAT_EDGE_GAIN, 20) - which
            straddles the Mish threshold 20 - and as drawn; the two layers of the time embedding scaled so that both Mish calls of
            the time table see values below -20 and above 45 (n (n + 2), n = e^x, leaves float32 at x ~ 44.4)

The constants were tuned on the CPU until tests/test_hostile_weights_host.py held in every block of every architecture; the
conditions asserted there are the contract, not the constants.
"""
import numpy as np
import torch

from edmp_amd import weights as W

KINDS = ("offset", "flat", "dead", "saturate")
GROUPS = 8
OFFSET = 25.0
SAT_GAIN, SAT_BIAS, SAT_EDGE_GAIN = 30.0, 30.0, 3.0
TIME_SCALE_1, TIME_SCALE_3 = 60.0, 3.0  # on time_embedding.time_mlp.1.weight / .3.weight


# what the two test modules share: the architectures (names of tests/plan_record.archs()), the seed, the time steps, the batches
ARCHS = ("A2", "A3", "A10", "FULL", "TINY")
SEED = 31
TS = (255, 1)
B_GPU, B_HOST = 37, 5  # 37: ragged against the 4-, 16- and 32-sample tiles; the host test censuses the first five of those rows


def arch_state_dict(arch, kind):
    from tests import plan_record as R

    cin, td, dims, _ = R.archs()[arch]
    return hostile_state_dict(kind, SEED, cin, td, dims)


def arch_input(arch):
    """(B_GPU, input_dim, horizon) float32, the same for every family"""
    from tests import plan_record as R

    cin, _, _, n = R.archs()[arch]
    return (np.random.RandomState(1000 + SEED).standard_normal((B_GPU, cin, n)) * 1.5).astype(np.float32)


def conv_blocks(sd):
    """the Conv1dBlock prefixes of a state dict, in its order: the block index of the rules above"""
    return [k[: -len(".block.0.weight")] for k in sd if k.endswith(".block.0.weight")]


def hostile_state_dict(kind, seed, input_dim, time_dim, dims):
    """name -> float32 ndarray: weights.init_state_dict(seed, ...) with the family's rule applied to every Conv1dBlock"""
    assert kind in KINDS, kind
    sd = W.init_state_dict(seed, input_dim, time_dim, dims)
    for bi, p in enumerate(conv_blocks(sd)):
        w, b = sd[p + ".block.0.weight"].astype(np.float64), sd[p + ".block.0.bias"].astype(np.float64)
        gamma, beta = sd[p + ".block.2.weight"].astype(np.float64), sd[p + ".block.2.bias"].astype(np.float64)
        C = w.shape[0]
        assert C % GROUPS == 0, (p, C)
        g = np.arange(C) // (C // GROUPS)
        if kind == "offset":
            b = b + OFFSET * (0.5 + g / 8.0) * np.where((g + bi) % 2 == 0, 1.0, -1.0)
        elif kind == "flat":
            s = 10.0 ** (-((g + bi) % 8) / 2.0)
            w, b = w * s[:, None, None], b * s
        elif kind == "dead":
            w[g == bi % 8], b[g == bi % 8] = 0.0, 0.0
        else:
            c = np.arange(C) % 4
            gamma = np.select([c == 0, c == 1, c == 2], [SAT_GAIN, -SAT_GAIN, SAT_EDGE_GAIN], gamma)
            beta = np.select([c == 0, c == 1, c == 2], [SAT_BIAS, -SAT_BIAS, 20.0], beta)
        for k, v in ((".block.0.weight", w), (".block.0.bias", b), (".block.2.weight", gamma), (".block.2.bias", beta)):
            sd[p + k] = np.ascontiguousarray(v, dtype=np.float32)
    if kind == "saturate":
        for k, s in (("time_embedding.time_mlp.1.weight", TIME_SCALE_1), ("time_embedding.time_mlp.3.weight", TIME_SCALE_3)):
            sd[k] = np.ascontiguousarray(sd[k].astype(np.float64) * s, dtype=np.float32)
    return sd


def unclamped_rational_mish(x):
    """x n (n + 2) / (n (n + 2) + 2), n = e^x, as the device's fast Mish would be without its clamp at 20: n (n + 2) overflows
    float32 at x ~ 44.4 and the ratio is inf / inf"""
    n = torch.exp(x)
    w = n * (n + 2)
    return x * (w / (w + 2))


# (family, program id of tests/instance_programs.program_id) -> the (tap, t) that stand above the 3 x torch-float32 bar of
# tests/test_gpu_hostile_activations.py without the epilogue being the cause (docs/LAB_NOTES.md section 15).  On
# `saturate` torch-float32 is within 1.1e-7 ... 2.3e-7 x rms of float64 at these taps (mid 1.2e-7 on A2; down4 / down5 / mid 2.3e-7 /
# 1.6e-7 / 1.1e-7 on FULL) - most outputs are gamma x + beta passed through a saturated Mish - and the K loops that add 5 x 512 ...
# 5 x 1024 products of activations with a large common sign into one fp32 accumulator stand above 3 x that: measured x3.16 (A2, generic
# kernels) and x3.63 / x3.36 / x3.14 (FULL, 16-sample fp32 tiles; the 32-sample tiles of the same epilogue x2.95 at most, every tap at
# t = 255 x2.94 at most).  On scratch builds with the launched copy's epilogue as (x - mean) s + beta and libm Mish the same taps measured
# x3.09 and x3.60 / x3.34 / x3.10.  tests/test_hostile_weights_host.py re-checks the claim on the CPU with the two emulations below.
KNOWN_K_LOOP_EXCESS = {
    ("saturate", "A2/NO_FUSED=1"): (("mid", 1),),
    ("saturate", "FULL/BF16X3=0,MS16=0x1f"): (("down4", 1), ("down5", 1), ("mid", 1)),
}


# ---- float32 emulations of the two places a device kernel differs from torch's CPU arithmetic (where an error excess comes from) -------
def clamped_rational_mish(x):
    """the device's fast Mish (csrc/common.h: mish_fast / mish_fast2) in the tensor's own precision: n = 2^(min(x, 20) log2 e),
    w = n (n + 2), x (w / (w + 2)) with the division as a multiplication by the reciprocal"""
    n = torch.exp2(torch.clamp(x, max=20.0) * 1.44269504088896340736)
    w = n * (n + 2.0)
    return x * (w * torch.reciprocal(w + 2.0))


def device_form_group_norm(x, gamma, beta):
    """the epilogue copies' GroupNorm in the tensor's own precision: mean, then the variance of the differences (two passes),
    rstd = 1 / sqrt(var + 1e-5), and x s + (beta - s mean) with s = rstd gamma - the cancelling form"""
    B, C, L = x.shape
    g = x.reshape(B, GROUPS, -1)
    n = g.shape[2]
    mean = g.sum(dim=2, keepdim=True) / n
    var = ((g - mean) ** 2).sum(dim=2, keepdim=True) / n
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    s = rstd.expand_as(g).reshape(B, C, L) * gamma[None, :, None]
    return x * s + (beta[None, :, None] - s * mean.expand_as(g).reshape(B, C, L))


def serial_k_conv(x, w, b):
    """a k = 5 'same' convolution whose 5 Cin products per output are added one after the other into ONE accumulator of the tensor's
    own precision, as a matrix-pipe K loop does - torch's CPU convolution sums in blocks"""
    B, Cin, L = x.shape
    assert w.shape[1:] == (Cin, 5)
    xp = torch.nn.functional.pad(x, (2, 2))
    acc = b[None, :, None].expand(B, w.shape[0], L).clone()
    for ci in range(Cin):
        for k in range(5):
            acc += xp[:, ci, None, k:k + L] * w[None, :, ci, k, None]
    return acc


def oracle_forward(sd, x, t, dtype=torch.float32, gn_eps=None, mish_fn=None, observer=None, gn_fn=None, conv_fn=None):
    """(eps, taps) of oracle.edmp_oracle.unet_forward in `dtype` as ndarrays; gn_eps / mish_fn / gn_fn / conv_fn replace GroupNorm's
    eps / Mish / the Conv1dBlocks' GroupNorm / their k = 5 convolution in every layer (through the oracle's observer - without any of
    them, and without an observer, the default path runs)"""
    from oracle import edmp_oracle as O

    if observer is None and any(v is not None for v in (gn_eps, mish_fn, gn_fn, conv_fn)):
        observer = O.ForwardObserver()
    if gn_eps is not None:
        observer.gn_eps = gn_eps
    if mish_fn is not None:
        observer.mish_fn = mish_fn
    if gn_fn is not None:
        observer.gn_fn = gn_fn
    if conv_fn is not None:
        observer.conv_fn = conv_fn
    time_dim = int(np.shape(sd["time_embedding.time_mlp.1.weight"])[1])
    tsd = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    tr = {}
    with torch.no_grad():
        y = O.unet_forward(tsd, torch.as_tensor(x).to(dtype), torch.tensor([float(t)], dtype=dtype), time_dim, trace=tr, observer=observer)
    return y.numpy(), {k: v.numpy() for k, v in tr.items()}


def _mish_stats(v):
    v = v.double().numpy().ravel()
    return {"min": float(v.min()), "max": float(v.max()), "above_20": float(np.mean(v > 20.0)), "below_m20": float(np.mean(v < -20.0)),
            "in_19_21": float(np.mean((v >= 19.0) & (v <= 21.0)))}


def regime_census(sd, x, t):
    """One float64 forward of the oracle.  {"blocks": {Conv1dBlock prefix: {"var": (B, 8) group variances of the GroupNorm input,
    "ratio": (B, 8) |mean| / std (inf where the variance is 0), "mish": {min, max, above_20, below_m20, in_19_21} of the Mish
    inputs}}, "time": {"time_embedding" | "time_mlp": the same Mish record for the two Mish calls of the time embedding}}"""
    from oracle import edmp_oracle as O

    blocks, time = {}, {}

    class Census(O.ForwardObserver):
        def on_gn_input(self, name, v):
            g = v.double().reshape(v.shape[0], GROUPS, -1)
            var, mu = g.var(dim=2, unbiased=False).numpy(), g.mean(dim=2).numpy()
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(var > 0, np.abs(mu) / np.sqrt(var), np.inf)
            blocks[name] = {"var": var, "ratio": ratio}

        def on_mish_input(self, name, v):
            (blocks[name] if name in blocks else time.setdefault(name, {}))["mish"] = _mish_stats(v)

    oracle_forward(sd, x, t, torch.float64, observer=Census())
    assert list(blocks) == conv_blocks(sd) and sorted(time) == ["time_embedding", "time_mlp"]
    return {"blocks": blocks, "time": {k: v["mish"] for k, v in time.items()}}
