"""The SDF guide with all three optional terms on the GPU against the record of the parent commit (tests/golden/sdf_terms_parent.json,
written by scripts/record_sdf_terms_parent.py --gpu from the cells of tests/sdf_terms_cells.py): the smallest ensemble that runs all four
gradient kernels on the same rows - one 'sdf' guide with a self, goal and sweep weight beside an 'sv' guide that normalises, 4 rows each,
L = 6 waypoints under a goal window of 8, three obstacles of which one is a cylinder - as a guide and as a scene batch of two.

Bit-equality and text-equality, no tolerance: the change this holds is to the host path alone.  The kernels are the parent's
instruction for instruction (profiles/sdf_terms_isa.json) and are handed the same bytes."""
import json

import pytest

from tests import sdf_terms_cells as cells

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    rec = json.load(open(cells.RECORD))
    assert "gpu" in rec, "the record holds no GPU cells: run scripts/record_sdf_terms_parent.py --gpu against the parent commit"
    return rec["gpu"]


def test_gradient_sumsq_and_reports_of_a_guide(parent):
    got = json.loads(json.dumps(cells.gpu_guide_cells()))
    assert set(got) == {"t=0", f"t={cells.T_CHECK}"} == set(parent["guide"])
    for t, want in parent["guide"].items():
        for k in want:
            assert got[t][k] == want[k], (t, k)
    assert got["t=0"]["gradient_sha256"] != got[f"t={cells.T_CHECK}"]["gradient_sha256"]


def test_run_and_reports_of_a_scene_batch(parent):
    got = json.loads(json.dumps(cells.gpu_batch_cells()))
    assert set(got) == set(parent["batch"])
    for k, want in parent["batch"].items():
        assert got[k] == want, k


def test_refusals_keep_their_code_and_text(parent):
    got = json.loads(json.dumps(cells.gpu_refusals()))
    assert set(got) == set(parent["refusals"]) and len(got) > 50
    assert {k: (v, parent["refusals"][k]) for k, v in got.items() if v != parent["refusals"][k]} == {}
    assert {v[0] for v in got.values()} == {0, -1, -3}  # argument and state refusals, and the one call that is none ("set_goal derived")
