"""GPU: the layer program and the packed weight image of every cell of tests/program_record.py against what the parent commit built
(tests/golden/unet_program_parent.json, written by scripts/record_program_parent.py), for equality: the image's SHA-256, per op the
kernel name, the issued and the bf16-pipe FLOPs and the reported kernel attributes, the five FLOP totals, every activation tap's (C, L)
or its absence, and a refusal's message.  Floats are compared as exact doubles.

The model build walks the architecture twice - a layout-only pass that sizes the image and the buffers, then the pass that packs and
writes the program (csrc/unet.hip) - and a packed image is loaded by the same two passes without the packing: the record holds the
passes to each other, and test_packed_image_loads_the_same_model holds the packed-load path to the repack path, forward bits included."""
import json
import os

import numpy as np
import pytest
import torch

from tests import plan_record as R
from tests import program_record as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record():
    """{"ARCH/setting": entry} of the parent commit"""
    with open(P.RECORD) as f:
        rec = json.load(f)
    assert rec["max_batch"] == P.MAX_BATCH
    return P.unpack(rec)


def test_the_record_covers_the_grid(record):
    assert sorted(record) == sorted(f"{a}/{s}" for a, s in P.cells())
    assert len(P.cells()) == 11 * 18 + 4


def _check(record, aid, settings):
    sd = P.state_dict(aid)
    bad = []
    for s in settings:
        want = record[f"{aid}/{s}"]
        got = json.loads(json.dumps(P.cell(aid, s, sd=sd)))  # as the record was written and read; floats survive exactly
        if got != want:
            bad.append((s, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))))
    assert not bad, (aid, bad)


@pytest.mark.parametrize("aid", P.SMALL)
def test_program_and_image_equal_the_parents(record, aid):
    _check(record, aid, R.SETTINGS)


def test_program_and_image_equal_the_parents_full(record):
    _check(record, "FULL", P.FULL_SETTINGS)


@pytest.mark.parametrize("aid", ("TINY", "A1"))
def test_packed_image_loads_the_same_model(record, aid, tmp_path):
    from edmp_amd import weights as W

    cin, _, dims, n = R.archs()[aid]
    a = P.build(aid, "default")
    d = str(tmp_path / "model")
    os.makedirs(d)
    a.pack(os.path.join(d, W.PACKED_NAME))
    b = P.build(aid, "default", model_dir=d)
    assert b._packed is not None and b._flat is None
    assert json.loads(json.dumps(P.describe(b))) == record[f"{aid}/default"]
    B = 3
    x = torch.tensor(np.random.RandomState(P.seed_of(aid)).standard_normal((B, cin, n)) * 1.5, dtype=torch.float32)
    shapes = P.tap_shapes(a)
    assert any(v != "absent" for v in shapes.values())
    for t in (255, 1):
        tt = torch.tensor([float(t)])
        ya = a(x, tt).cpu().numpy()
        ta = {w: a.activation(int(w), B).cpu().numpy() for w, v in shapes.items() if v != "absent"}
        yb = b(x, tt).cpu().numpy()
        assert np.isfinite(ya).all() and np.array_equal(ya, yb), t
        for w, v in ta.items():
            assert np.array_equal(v, b.activation(int(w), B).cpu().numpy()), (t, w)
