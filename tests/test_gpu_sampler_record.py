"""Diffusion.denoise_guided and denoise_guided_scenes against the record of the parent commit (tests/golden/sampler_parent.json, written by
scripts/record_sampler_parent.py from the cells of tests/sampler_cells.py): every noise form - the global NumPy stream, a host array, a
device tensor, a pinned tensor, a published PinnedNoiseStream, a DeviceNoise and, for one scene, noise="device" - crossed with every run
form - stopped early, warm-started with and without re-noising from one plan or one per row, unguided, unconditioned, row 0 kept, a device
result, graph replay with the call made twice, a one-rank all-reduce hook, the whole loop - and one cell per refusal.

Equality, no tolerance: the digest of every result's dtype, shape and bytes, whether it is a device tensor, the global RandomState after
the call and, per context, the sequence of library entry points - of the loop's own calls also every integer argument and which pointers
are null -; of a refusal its type, its text and what the library had been asked before it.  The change this holds is to the structure of
the two methods and of the host code under their entry points alone."""
import json

import pytest

from tests import sampler_cells as cells
from tests.util import T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return json.load(open(cells.RECORD))["cells"]


def test_the_record_exercises_everything(parent):
    """a cell that stops exercising an entry point, a noise form or a refusal fails here instead of passing"""
    assert list(parent) == sorted(cells.cell_names()) and len(set(cells.cell_names())) == len(parent)
    called = {c[0] for cell in parent.values() for ctx in cell["calls"].values() for c, _ in ctx if isinstance(c, list)}
    assert called == set(cells.ENTRY_POINTS) and len(cells.ENTRY_POINTS) == 12
    for form in cells.FORMS:
        runs = {name.split(":")[1]: set() for name in parent if name.startswith(form) and name not in cells.REFUSALS}
        for name in parent:
            if name.startswith(form) and name not in cells.REFUSALS:
                runs[name.split(":")[1]].add(name.split(":")[2])
        single = form == "single"
        assert set(runs) == set(cells.RUNS) - (set() if single else {"sharded"}), form
        every = set(cells.NOISES) - (set() if single else {"string"})
        assert set().union(*runs.values()) == every and runs["stop"] == every and runs["full"] == set(cells.FULL), form
        assert all(v >= every - {"string"} for k, v in runs.items() if k not in ("full", "sharded")), form
    for name, cell in parent.items():
        if name in cells.REFUSALS:
            assert cell["error"] is not None and cell["error"][0] in ("ValueError", "EdmpError") and cell["error"][1] and "results" not in cell, name
            assert not cell["calls"]["lane1"], name
        else:
            assert len(cell["results"]) == (2 if ":graph_twice:" in name else 1) and cell["calls"]["base"] and not cell["calls"]["lane1"], name
            assert all(r["device"] == ("device_result" in name) for r in cell["results"]), name
    texts = [parent[name]["error"][1] for name in cells.REFUSALS]
    # six raise statements of _check_run and _check_warm are reached from both forms and give one text each, and the single form's late shape check
    # words a pinned and a host stream alike: every other refusal has a text of its own
    assert len(set(texts)) == len(texts) - 7
    guided_steps = sum(1 for t in range(T, T - cells.STEPS, -1) if t % 2 == 0 and t >= 5)
    assert all(parent[f"single:sharded:{n}"]["hook"] == {"kind": "python callback (ctypes -> torch.distributed)", "calls": guided_steps} for n in ("host", "device", "pinned", "stream"))


@pytest.mark.parametrize("name", cells.cell_names())
def test_call_equals_the_parent(parent, name):
    got, want = cells.evaluate(name), parent[name]
    assert set(got) == set(want)
    for part in sorted(want):
        if part != "calls":
            assert got[part] == want[part], part
    for ctx in want["calls"]:
        assert got["calls"][ctx] == want["calls"][ctx], ctx
