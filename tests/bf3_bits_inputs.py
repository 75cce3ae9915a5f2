"""The forwards of tests/test_gpu_bf3_bits.py and scripts/record_bf3_parent_bits.py (one definition for the recorder and the test).

One UNet forward at B = 33 and t = 37 under the default program on three architectures:
  full  dims (32, 64, 128, 256, 512, 512): all 16 listed bf16x3 instances (csrc/kernel_instances.h), K loops of 2, 4, 8, 16 and 32 chunks
  nk1   dims (32, 32, 128):  bf3_conv_kernel<0, 16, 32, 16, 13, true> reads 32 input channels: a K loop of ONE chunk
  nk3   dims (32, 96, 128):  the same instance reads 96 input channels: three chunks (an odd count)
B = 33: one full tile and a one-row tile of the 32-sample instances, two full tiles and a one-row tile of the 16-sample ones.

What is kept of a forward: eps whole; of every activation tap the program has an HBM copy of, the SHA-256 of its float32 bytes (as strong
a bit-for-bit check as the array, at 64 bytes instead of ~100 KB: the taps of the three forwards are 4 MB) and rows ROWS whole - the
first and last row of each tile - so that a mismatch can be looked at."""
import hashlib

import numpy as np

B = 33
T_STEP = 37
ROWS = (0, 15, 16, 31, 32)
INPUT_DIM, TIME_DIM, HORIZON = 7, 32, 50
ARCHS = {  # name -> (dims, weight seed)
    "full": ((32, 64, 128, 256, 512, 512), 61),
    "nk1": ((32, 32, 128), 62),
    "nk3": ((32, 96, 128), 63),
}
# the bf16x3 instances each program has to hold (kernel names as edmp_unet_plan_describe prints them)
BF3_FULL = tuple(f"bf3_conv_kernel<{k}, {ms}, {cg}, {gs}, {l}, {r}>" for k, ms, cg, gs, l, r in (
    (0, 32, 32, 32, 7, "true"), (0, 32, 32, 32, 7, "false"), (0, 16, 32, 16, 7, "true"), (0, 16, 32, 16, 7, "false"),
    (0, 16, 32, 16, 13, "true"), (0, 16, 32, 16, 13, "false"), (1, 32, 32, 32, 7, "false"), (2, 32, 32, 32, 4, "false"),
    (1, 32, 32, 32, 4, "false"), (2, 32, 32, 32, 2, "false"), (1, 16, 32, 16, 13, "false"), (2, 16, 32, 16, 7, "false"),
    (0, 32, 64, 64, 4, "true"), (0, 32, 64, 64, 4, "false"), (0, 32, 32, 32, 4, "true"), (0, 32, 32, 32, 4, "false")))
BF3_SMALL = ("bf3_conv_kernel<0, 16, 32, 16, 13, true>", "bf3_conv_kernel<0, 16, 32, 16, 13, false>")


def taps_of(dims):
    return list(range(len(dims))) + [100] + [200 + j for j in range(len(dims) - 1)]


def state_dict(name):
    from edmp_amd import weights as W

    dims, seed = ARCHS[name]
    return W.init_state_dict(seed, INPUT_DIM, TIME_DIM, dims)


def x_input(name):
    return (np.random.RandomState(3300 + ARCHS[name][1]).standard_normal((B, INPUT_DIM, HORIZON)) * 1.5).astype(np.float32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def forward(name, device="cuda:0"):
    """(net, eps, {tap: array}) of the forward, on whichever edmp_amd package the interpreter imports"""
    import torch

    from edmp_amd import _capi
    from edmp_amd.temporalunet import TemporalUNet

    dims, _ = ARCHS[name]
    net = TemporalUNet(None, INPUT_DIM, TIME_DIM, device, dims=dims, state_dict=state_dict(name), max_batch=B, horizon=HORIZON)
    eps = net(torch.from_numpy(x_input(name)), torch.tensor([float(T_STEP)])).cpu().numpy()
    taps = {}
    for w in taps_of(dims):
        try:
            taps[w] = net.activation(w, B).cpu().numpy()
        except _capi.EdmpError:  # no HBM copy of this tap in the program (a merged level)
            continue
    return net, eps, taps


def record(name, device="cuda:0"):
    """the fixture's entries for one architecture"""
    net, eps, taps = forward(name, device)
    net._bind()
    out = {f"{name}_eps": eps, f"{name}_ops": np.array([n for n, _, _, _ in net.ctx.prof_ops()]), f"{name}_taps": np.array(sorted(taps), dtype=np.int64)}
    for w, a in taps.items():
        out[f"{name}_tap{w}_sha256"] = np.array(digest(a))
        out[f"{name}_tap{w}_rows"] = np.ascontiguousarray(a[list(ROWS)])
    return out
