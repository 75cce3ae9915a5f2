"""The host path of the SDF guide's optional terms against the record of the parent commit (tests/golden/sdf_terms_parent.json, written by
scripts/record_sdf_terms_parent.py from the cells of tests/sdf_terms_cells.py): every array that guide_cfg, guide.sdf_tables,
guide.scene_batch_tables and dist.shard_guide_cfgs hand on keeps its key, place, dtype, shape and bytes, and every odd input keeps its
verdict - accepted (with what came of it) or the exception's type."""
import json
import os
import re
import warnings

import pytest

from tests import sdf_terms_cells as cells


@pytest.fixture(scope="module")
def parent():
    return json.load(open(cells.RECORD))["host"]


def test_every_array_keeps_its_key_dtype_shape_and_bytes(parent):
    got = json.loads(json.dumps(cells.host_cells()))
    assert list(got) == list(cells.GUIDE_SETS) and set(got) == set(parent["cells"])
    for name, want in parent["cells"].items():
        for part in want:
            assert got[name][part] == want[part], (name, part)


@pytest.mark.parametrize("family", ["cfg_probes", "table_probes"])
def test_every_odd_input_keeps_its_verdict(parent, family):
    probes = getattr(cells, family)()
    assert set(probes) == set(parent[family]) and len(probes) > 300
    kinds = {v.split()[0] for v in parent[family].values()}
    assert kinds == {"accepted", "ValueError", "TypeError"}  # the probes reach every kind of verdict
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (casting a probe's complex or NaN entries warns, on the parent as here)
        got = {k: cells.verdict(f) for k, f in probes.items()}
    assert {k: v for k, v in got.items() if v != parent[family][k]} == {}


def test_the_term_keys_are_spelled_in_one_module():
    """each of the seven term keys stands as a string literal in exactly one file of the package: the term table (docstrings and comments aside)"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "edmp_amd")
    for cfg_key, _ in cells.TERM_KEYS:
        hits = []
        for fn in sorted(os.listdir(root)):
            if fn.endswith(".py"):
                src = re.sub(r'"""(?:.|\n)*?"""', "", open(os.path.join(root, fn)).read())
                src = re.sub(r"#.*", "", src)
                if re.search(r"[\"']" + cfg_key + r"[\"']", src):
                    hits.append(fn)
        assert hits == ["sdf_terms.py"], (cfg_key, hits)
