"""Which kernel instance every layer of every model picks, under every builder switch, held to a committed record - on the CPU.

tests/golden/unet_plan_record.json was written by scripts/gen_plan_record.py from the selection code as it stood BEFORE the instance
table replaced the per-site ladders of csrc/unet.hip; edmp_unet_plan_describe (host-only) must reproduce it cell by cell: layout id
of the packed image, its size, the count of each kernel name and the hash of the ordered name list.  tests/test_gpu_archs.py ties the
described names to what a bound model launches."""
import json

import pytest

from tests import plan_record as R

ARCHS = R.archs()


@pytest.fixture(scope="module")
def record():
    with open(R.RECORD) as f:
        return json.load(f)


def test_the_record_covers_the_grid(record):
    assert set(record["cells"]) == set(ARCHS)
    for a in ARCHS:
        assert set(record["cells"][a]) == set(R.SETTINGS), a


@pytest.mark.parametrize("arch", list(ARCHS))
def test_plan_matches_the_record(record, arch):
    for sname, setting in R.SETTINGS.items():
        layout, n_packed, pi = record["cells"][arch][sname]
        plan = record["plans"][pi]
        want = {"layout": layout, "n_packed": n_packed, "counts": {record["names"][i]: c for i, c in plan["counts"]}, "sha256": plan["sha256"]}
        assert R.describe(ARCHS[arch], setting) == want, (arch, sname)


def test_describe_leaves_the_environment_alone_and_refuses_a_bad_desc():
    import os

    from edmp_amd import _capi

    before = dict(os.environ)
    R.describe(ARCHS["TINY"], {"EDMP_BF16X3": "0"})
    assert dict(os.environ) == before
    with pytest.raises(_capi.EdmpError, match="n_levels"):
        _capi.plan_describe(7, 32, (32,), 50, 255)
