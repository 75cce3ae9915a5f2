"""GPU: after a change to where the bf16x3 K loop (csrc/bf3.hip) places its memory instructions, the FULL architecture computes, bit
for bit, what it computed at the commit recorded in tests/golden/bf3_forward_parent.json (scripts/record_bf3_forward_parent.py).

The forwards are those of tests/bf3_forward_inputs.py: one model with max_batch 33, forward at t = 255 and t = 1 for B = 33 (a full
32-row tile and a one-row ragged one) and B = 17 (a full and a ragged 16-row tile) - the smallest batches that run every bf16x3
instance at both tile heights with clamped rows.  The output and every activation tap with an HBM copy are compared by shape and
SHA-256: a reordering that changes any accumulator's MFMA sequence, a staged value or a stage address changes a hash.  No tolerance.

(tests/test_gpu_bf3_bits.py holds the same kernels to an earlier fixture at B = 33, t = 37 and to the oracle; this file adds the second
batch, the two ends of the time axis and the FULL model of tests/program_record.py.)"""
import json
import os

import pytest

from tests import bf3_forward_inputs as I
from tests.bf3_bits_inputs import BF3_FULL

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", I.RECORD_NAME)
_NET = []


def _net():
    if not _NET:
        net = I.build()
        net._bind()
        _NET.append(net)
    return _NET[0]


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_program_runs_every_bf16x3_instance():
    g = _golden()
    assert g["max_batch"] == I.MAX_BATCH
    ops = [n for n, _, _, _ in _net().ctx.prof_ops()]
    assert ops == g["ops"], "the program changed: re-record the fixture from the parent of the change under test"
    missing = [n for n in BF3_FULL if n not in ops]
    assert not missing, missing


@pytest.mark.parametrize("b,t", I.CASES)
def test_forward_equals_the_parent_commits_hashes(b, t):
    g = _golden()
    want = g["cases"][I.key(b, t)]
    got = I.forward(_net(), b, t)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    bad = [f"{n}: shape {got[n]['shape']} sha256 {got[n]['sha256'][:16]}, parent {want[n]['shape']} {want[n]['sha256'][:16]}" for n in sorted(want) if got[n] != want[n]]
    assert not bad, f"[B = {b}, t = {t}] against parent commit {g['parent_commit']}:\n" + "\n".join(bad)
