"""The forwards of tests/test_gpu_bf3_forward_bits.py and scripts/record_bf3_forward_parent.py (one definition for the recorder and the test).

The FULL architecture of tests/program_record.py (its seeded state dict, default program: all 16 listed bf16x3 instances), built once
with max_batch 33, run forward at t = 255 and t = 1 for B = 33 and B = 17:
  B = 33: one full tile and a one-row ragged tile of the 32-sample instances (two full tiles and a one-row tile of the 16-sample ones);
  B = 17: a full and a one-row ragged tile of the 16-sample instances (one 17-row ragged tile of the 32-sample ones).
A ragged tile's rows past B are the clamped ones (the staging waves re-read row B - 1, the epilogue stores nothing for them).

What is kept of a forward: shape and SHA-256 of the float32 bytes of eps and of every activation tap the program has an HBM copy of."""
import hashlib

import numpy as np

MAX_BATCH = 33
CASES = tuple((b, t) for b in (33, 17) for t in (255, 1))  # (B, t)
RECORD_NAME = "bf3_forward_parent.json"


def key(b, t):
    return f"B{b}_t{t}"


def x_input(b, t, cin, horizon):
    return (np.random.RandomState(7000 + 10 * b + t).standard_normal((b, cin, horizon)) * 1.5).astype(np.float32)


def entry(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return {"shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def build(device="cuda:0"):
    from edmp_amd.temporalunet import TemporalUNet
    from tests import plan_record as R
    from tests import program_record as P

    cin, td, dims, n = R.archs()["FULL"]
    return TemporalUNet(None, cin, td, device, dims=dims, state_dict=P.state_dict("FULL"), max_batch=MAX_BATCH, horizon=n)


def forward(net, b, t):
    """{"eps": entry, "tap<id>": entry ...} of one forward, on whichever edmp_amd package the interpreter imports"""
    import torch

    from edmp_amd import _capi
    from tests import program_record as P

    x = x_input(b, t, net.input_dim, net.horizon)
    out = {"eps": entry(net(torch.from_numpy(x), torch.tensor([float(t)])).cpu().numpy())}
    for w in P.tap_ids(len(net.dims)):
        try:
            out[f"tap{w}"] = entry(net.activation(w, b).cpu().numpy())
        except _capi.EdmpError:  # no HBM copy of this tap in the program (a merged level)
            continue
    return out


def record(device="cuda:0"):
    """the fixture's body: the program's op names (the instances the forwards ran) and the entries of every case"""
    net = build(device)
    net._bind()
    return {"ops": [n for n, _, _, _ in net.ctx.prof_ops()], "cases": {key(b, t): forward(net, b, t) for b, t in CASES}}
