"""The paired workgroups of the 512-channel bf16x3 resamplers (bf3.hip: Bf3Cfg::PAIRABLE, launch_bf3_t's pairing rule) give the bits of
the unpaired ones.

Only the full architecture (32, 64, 128, 256, 512, 512) reaches bf3_conv_kernel<1, 32, 32, 32, 4, false> (k3s2, 512 -> 512, L 4 -> 2)
and bf3_conv_kernel<2, 32, 32, 32, 2, false> (ConvTranspose, 512 -> 512, L 2 -> 4).  Each has 512 / 32 = 16 channel groups; a launch
pairs them iff 16 x ceil(B / 32) exceeds the device's CU count.  B = 545 (17 full sample tiles + one row: 288 workgroups unpaired) and
B = 529 (16 tiles + 17 rows: 272) pair on a device of fewer than 272 CUs, B = 33 (32 workgroups) never does - and the B = 33 forward of
the default program is what tests/test_gpu_bf3_bits.py ties to the parent commit's bits.  A UNet row does not depend on the rows beside
it, so equal inputs must give equal rows, bit for bit, in eps and in every activation tap: no tolerance anywhere in this file.

What was compared (batches, arrays, elements differing) goes to profiles/bf3_paired_resamplers.json, beside the timings."""
import json
import os

import numpy as np
import pytest

from tests import bf3_bits_inputs as BI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_BIG, B_HALF, B_SMALL, TAIL0 = 545, 529, 33, 512
PAIRED_OPS = ("bf3_conv_kernel<1, 32, 32, 32, 4, false>", "bf3_conv_kernel<2, 32, 32, 32, 2, false>")
CHANNEL_GROUPS = 16  # 512 output channels / 32


@pytest.fixture(scope="module")
def runs():
    """{name: (eps, {tap: array})} of the four forwards: one network, seeded weights, the default program"""
    import torch

    from edmp_amd import _capi
    from edmp_amd.temporalunet import TemporalUNet

    dims, _ = BI.ARCHS["full"]
    net = TemporalUNet(None, BI.INPUT_DIM, BI.TIME_DIM, "cuda:0", dims=dims, state_dict=BI.state_dict("full"), max_batch=B_BIG, horizon=BI.HORIZON)
    x = (np.random.RandomState(54500).standard_normal((B_BIG, BI.INPUT_DIM, BI.HORIZON)) * 1.5).astype(np.float32)

    def forward(xs):
        n = xs.shape[0]
        eps = net(torch.from_numpy(np.ascontiguousarray(xs)), torch.tensor([float(BI.T_STEP)])).cpu().numpy()
        taps = {}
        for w in BI.taps_of(dims):
            try:
                taps[w] = net.activation(w, n).cpu().numpy()
            except _capi.EdmpError:  # no HBM copy of this tap in the program (a merged level)
                continue
        return eps, taps

    out = {"big": forward(x), "half": forward(x[:B_HALF]), "head": forward(x[:B_SMALL]), "tail": forward(x[TAIL0:B_BIG])}
    net._bind()
    out["ops"] = [n for n, _, _, _ in net.ctx.prof_ops()]
    return out


def _differing(a, b, rows_a, rows_b):
    """(arrays compared, elements differing) between rows rows_a of run a and rows rows_b of run b, eps and every tap"""
    (eps_a, taps_a), (eps_b, taps_b) = a, b
    assert sorted(taps_a) == sorted(taps_b) and taps_a, (sorted(taps_a), sorted(taps_b))
    pairs = [(eps_a, eps_b)] + [(taps_a[w], taps_b[w]) for w in sorted(taps_a)]
    bad = 0
    for u, v in pairs:
        u, v = u[rows_a], v[rows_b]
        assert u.shape == v.shape and u.size > 0, (u.shape, v.shape)
        assert np.isfinite(u).all()
        bad += int(np.count_nonzero(u.view(np.uint32) != v.view(np.uint32)))
    return len(pairs), bad


def _note(key, entry):
    path = os.path.join(ROOT, "profiles", "bf3_paired_resamplers.json")
    try:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.setdefault("bit_comparison", {})[key] = entry
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    except OSError:  # a read-only checkout: the assertions below are the test
        pass


def test_the_large_batches_are_past_the_pairing_threshold(runs):
    """the test must not pass by testing nothing: both resamplers are in the program, and 16 groups x 17 tiles already outnumber the CUs"""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus < CHANNEL_GROUPS * 17, cus
    assert CHANNEL_GROUPS * ((B_SMALL + 31) // 32) <= cus
    for name in PAIRED_OPS:
        assert name in runs["ops"], (name, runs["ops"])


@pytest.mark.parametrize("key,a,b,rows_a,rows_b", [
    # paired equals unpaired, by prefix: the first 33 rows of B = 545 against the B = 33 forward of the same inputs
    ("prefix", "big", "head", slice(0, B_SMALL), slice(0, B_SMALL)),
    # ... at the short tile: row 544 is alone in its tile (the second row block all clamped rows; the store guard b < B decides)
    ("short_tile", "big", "tail", slice(TAIL0, B_BIG), slice(0, B_SMALL)),
    # a half tile: B = 529 has one real row in the last tile's second row block
    ("half_tile", "half", "big", slice(TAIL0, B_HALF), slice(TAIL0, B_HALF)),
])
def test_paired_rows_equal_unpaired_rows(runs, key, a, b, rows_a, rows_b):
    arrays, bad = _differing(runs[a], runs[b], rows_a, rows_b)
    sizes = {"big": B_BIG, "half": B_HALF, "head": B_SMALL, "tail": B_SMALL}
    print(f"[{key}] B = {sizes[a]} rows {rows_a.start}..{rows_a.stop - 1} against B = {sizes[b]} rows {rows_b.start}..{rows_b.stop - 1}: {arrays} arrays, {bad} elements differ")
    _note(key, {"batches": [sizes[a], sizes[b]], "rows": [[rows_a.start, rows_a.stop], [rows_b.start, rows_b.stop]], "arrays": arrays, "elements_differing": bad})
    assert bad == 0
