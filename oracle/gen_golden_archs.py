"""G16: pin the oracle's TemporalUNet against the UNMODIFIED reference on the architectures the C-ABI accepts beyond the
TINY / FULL networks of G8, and emit tests/golden/g16_unet_archs.npz — TEST INFRASTRUCTURE ONLY.

Run where the reference checkout is available (oracle.ref_harness.REF):   python -m oracle.gen_golden_archs
For every architecture A1..A10 it (1) builds the reference TemporalUNet with the seeded weights of
``edmp_amd.weights.init_state_dict``, (2) runs it on a seeded x (B = 3) at t = 255, 37, 1 in float32 and, module and
inputs in ``.double()``, in float64, (3) asserts that ``oracle.edmp_oracle.unet_forward`` reproduces both bit for bit and
(4) stores x and the reference outputs.  It also records the reference's Diffusion schedule at T = 2, 50, 1000 and the two
architectures the reference itself cannot run (R2, R3: the skip and the up-sampled lengths differ) as refusals.
The fixture holds data only (arrays, architecture parameters, the reference's error text); no reference source.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from edmp_amd import weights as W  # noqa: E402
from oracle import edmp_oracle as O  # noqa: E402
from oracle import ref_harness  # noqa: E402
from oracle.gen_golden import check, save  # noqa: E402

# id -> (dims, input_dim, time_dim, horizon); the seed of the weights is 100 + the number of the id
ARCHS = {
    "A1": ((32, 64, 128, 256), 7, 32, 50),
    "A2": ((32, 64, 128, 256, 512), 7, 32, 50),
    "A3": ((32, 64), 7, 32, 50),
    "A4": ((32, 64, 128, 256, 512, 512, 512), 7, 32, 50),
    "A5": ((24, 40, 72, 136), 7, 32, 50),
    "A6": ((8, 24, 56), 3, 16, 50),
    "A7": ((32, 64, 128, 256), 2, 64, 50),
    "A8": ((32, 64, 128, 256), 8, 4, 50),
    "A9": ((32, 64, 128, 256), 7, 32, 64),
    "A10": ((48, 64, 128), 7, 32, 48),
}
# architectures the reference cannot run: the up path's lengths do not meet the skips'
REFUSED = {
    "R2": ((32, 64, 128, 256, 512, 512, 512, 512), 7, 32, 50),
    "R3": ((16, 32, 64, 64), 7, 32, 32),
}
TS = (255, 37, 1)
SCHED_TS = (2, 50, 1000)
B = 3


def seed_of(aid):
    return 100 + int(aid[1:])


def main():
    torch.manual_seed(0)
    refd, _ = ref_harness.install(O.PLACEHOLDER_LINK_EXTENTS)
    tmp = tempfile.mkdtemp(prefix="edmp_models_")
    rs = np.random.RandomState(16)
    out = {"ids": np.array(list(ARCHS)), "refused_ids": np.array(list(REFUSED)), "ts": np.array(TS), "sched_Ts": np.array(SCHED_TS)}
    print("G16 TemporalUNet architectures")
    for aid, (dims, cin, td, n) in ARCHS.items():
        seed = seed_of(aid)
        sd = W.init_state_dict(seed, cin, td, dims)
        net = refd.TemporalUNet(model_name=os.path.join(tmp, aid), input_dim=cin, time_dim=td, device="cpu", dims=dims)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        net.train(False)
        x = torch.tensor(rs.standard_normal((B, cin, n)), dtype=torch.float32)
        sd32 = {k: torch.from_numpy(v) for k, v in sd.items()}
        sd64 = {k: v.double() for k, v in sd32.items()}
        arrs = dict(dims=np.array(dims), input_dim=np.array(cin), time_dim=np.array(td), horizon=np.array(n), seed=np.array(seed), x=x.numpy())
        for t in TS:
            tt = torch.tensor([float(t)])
            with torch.no_grad():
                y32 = net(x, tt)
                o32 = O.unet_forward(sd32, x, tt, td)
            check(f"G16.{aid} f32 t={t}", o32.numpy(), y32.numpy())
            arrs[f"eps32_t{t}"] = y32.numpy()
        net.double()
        for t in TS:
            tt = torch.tensor([float(t)], dtype=torch.float64)
            with torch.no_grad():
                y64 = net(x.double(), tt)
                o64 = O.unet_forward(sd64, x.double(), tt, td)
            assert y64.dtype == torch.float64
            check(f"G16.{aid} f64 t={t}", o64.numpy(), y64.numpy())
            arrs[f"eps64_t{t}"] = y64.numpy()
        out.update({f"{aid}_{k}": v for k, v in arrs.items()})
    print("G16 architectures the reference refuses")
    for rid, (dims, cin, td, n) in REFUSED.items():
        sd = W.init_state_dict(seed_of(rid), cin, td, dims)
        net = refd.TemporalUNet(model_name=os.path.join(tmp, rid), input_dim=cin, time_dim=td, device="cpu", dims=dims)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        net.train(False)
        try:
            with torch.no_grad():
                net(torch.zeros(1, cin, n), torch.tensor([1.0]))
        except RuntimeError as e:
            msg = str(e).splitlines()[0]
        else:
            raise AssertionError(f"{rid}: the reference ran {dims} at horizon {n}")
        print(f"  [G16.{rid}] {dims} at N = {n}: {msg}")
        out.update({f"{rid}_dims": np.array(dims), f"{rid}_input_dim": np.array(cin), f"{rid}_time_dim": np.array(td),
                    f"{rid}_horizon": np.array(n), f"{rid}_error": np.array(msg)})
    print("G16 Diffusion schedules")
    for T in SCHED_TS:
        dif = refd.Diffusion(T=T, device="cpu")
        b, a, ab = O.schedule(T)
        check(f"G16.beta T={T}", b, dif.beta)
        check(f"G16.alpha T={T}", a, dif.alpha)
        check(f"G16.alpha_bar T={T}", ab, dif.alpha_bar)
        out.update({f"sched{T}_beta": np.asarray(dif.beta), f"sched{T}_alpha": np.asarray(dif.alpha), f"sched{T}_alpha_bar": np.asarray(dif.alpha_bar)})
    save("g16_unet_archs", **out)


if __name__ == "__main__":
    main()
