"""infer_serial.run against the record of the parent commit (tests/golden/driver_parent.json, written by scripts/record_driver_parent.py
from the cells of tests/driver_cells.py): per cell one run of two or three scenes - plain, every option at once, the report alone, the
device noise source and a problem set solved from its target poses, each through the serial loop and through a scene group (a leftover
group of one included), and two scenes in flight.

Equality, no tolerance: every result's keys in order, types and values (floats by their bits, arrays by a digest; wall-clock values by
key and type), the order of the `timings` keys and their texts, every printed line, the summary, the global RandomState after the run
and, per context, the sequence of library entry points.  The change this holds is to the driver's structure alone."""
import json

import pytest

from tests import driver_cells as cells

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return json.load(open(cells.RECORD))["cells"]


def test_the_record_exercises_every_option(parent):
    """a cell that stops exercising an option fails here instead of passing: no cell is empty, every optional key occurs"""
    assert set(parent) == set(cells.CELLS)
    for name, cell in parent.items():
        assert len(cell["scenes"]) == cells.CELLS[name][1] and len(cell["printed"]) > len(cell["scenes"]) and cell["calls"]["base"], name
        assert all(len(s["keys"]) >= 17 and s["values"] and s["timings"] for s in cell["scenes"]), name
    keys = {k for cell in parent.values() for s in cell["scenes"] for k in s["keys"]}
    timings = {k for cell in parent.values() for s in cell["scenes"] for k, _ in s["timings"]}
    assert set(cells.OPTIONAL_KEYS) <= keys and set(cells.OPTIONAL_TIMINGS) <= timings
    assert parent["plain_in_flight"]["calls"]["lane1"] and not parent["plain_serial"]["calls"]["lane1"]
    assert {s["values"]["scenes_in_launch"] for s in parent["all_group"]["scenes"]} == {1, 2}  # (the leftover group of one)


@pytest.mark.parametrize("name", list(cells.CELLS))
def test_run_equals_the_parent(parent, name, tmp_path):
    got = json.loads(json.dumps(cells.evaluate(name, tmp_path)))
    want = parent[name]
    assert set(got) == set(want)
    assert len(got["scenes"]) == len(want["scenes"])
    for i, (g, w) in enumerate(zip(got["scenes"], want["scenes"])):
        for part in ("keys", "types", "timings", "values"):
            assert g[part] == w[part], (i, part)
    for part in ("printed", "summary", "random_state"):
        assert got[part] == want[part], part
    for ctx in want["calls"]:
        assert got["calls"][ctx] == want["calls"][ctx], ctx
