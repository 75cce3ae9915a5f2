"""GPU: the three exact f64 checks (success_rows_kernel, shortcut_rows_kernel, self_collision_rows_kernel; csrc/linkbox.h) on the cases of
tests/overlap_inputs.py, in each of which ONE step of the overlap tests decides: each of the 15 separating axes as the sole separator and
as the tightest axis of an overlapping pair, on every link box and between link boxes; the cylinder test's axis line, each of its 12
clipped edges and each of its 24 cap-plane segments, with and without the exchange of the face's axes, and the exact zeros of an
axis-aligned pair.  tests/test_overlap_host.py holds the cases to their classes on the CPU.

Every case runs as the smallest input a kernel accepts and every comparison is an exact flag or index.  The success check (the cylinder
test as a call, its indexed form) sees the constant row of q; the shortcut stage (the inlined select form) a three-waypoint row whose one
candidate tests q.  The link cases run in scene batches of up to 16 one-obstacle scenes, boxes and cylinders mixed, and the first cases of
every family through single-scene guides as well.  Per-class counts (cases, wrong) are printed family by family; with
EDMP_OVERLAP_PARITY_OUT=<file> they are written there as JSON (profiles/overlap_parity.json comes from such a run)."""
import collections
import functools

import numpy as np
import pytest

from oracle import success_oracle as SO
from tests import overlap_inputs as OI
from tests import repair_inputs as RI
from tests import self_collision_inputs as SCI
from tests.sdf_gpu import DEV, recorder

pytestmark = pytest.mark.gpu
record, _write_records = recorder("overlap parity", "EDMP_OVERLAP_PARITY_OUT", "exact: every flag and index equals the class's truth")

LINK, SELF = OI.link_cases(), OI.self_cases()
GROUPS = OI.groups(LINK)
FAMILIES = sorted({c["family"] for c in LINK})
SELF_FAMILIES = sorted({c["family"] for c in SELF})
PER_FAMILY_SINGLE = 3


def make_guide(case, bind=True):
    """the one-row guide of a link case: its one obstacle and the placeholder link boxes of the host classifier"""
    from edmp_amd.guide import IntersectionVolumeGuide

    return IntersectionVolumeGuide(np.asarray(case["oc"])[None], DEV, RI.plain_cfgs(1), 1, link_mesh_extents=OI.EXTENTS,
                                   obstacle_kinds=np.array([case["kind"]], dtype=np.int32), bind=bind)


def singles():
    """the first PER_FAMILY_SINGLE cases of every family"""
    seen, out = collections.Counter(), []
    for c in LINK:
        if seen[c["family"]] < PER_FAMILY_SINGLE:
            seen[c["family"]] += 1
            out.append(c)
    return out


@pytest.fixture(scope="module")
def batch_results():
    """name -> dict(first, ok, tested, accepted): every link case once through the scene batches of its group"""
    from edmp_amd.guide import SceneBatch

    out = {}
    for group in GROUPS:
        batch = SceneBatch([make_guide(c, bind=False) for c in group])
        res = batch.success_rows(np.stack([OI.constant_row(c["q"])[None] for c in group]), substeps=1)
        cut = batch.shortcut_rows(np.stack([OI.shortcut_row(c["q"])[None] for c in group]), passes=1, substeps=1)
        assert res["first"].shape == (len(group), 1) and cut["tested"].shape == (len(group), 1) and res["within"].all()
        for s, c in enumerate(group):
            out[c["name"]] = dict(first=int(res["first"][s, 0]), ok=bool(res["ok"][s, 0]), tested=int(cut["tested"][s, 0]), accepted=int(cut["accepted"][s, 0]))
    return out


@pytest.fixture(scope="module")
def single_results():
    out = {}
    for c in singles():
        g = make_guide(c)
        res = g.success_rows(OI.constant_row(c["q"])[None], substeps=1)
        cut = g.shortcut_rows(OI.shortcut_row(c["q"])[None], passes=1, substeps=1)
        assert res["within"].all()
        out[c["name"]] = dict(first=int(res["first"][0]), ok=bool(res["ok"][0]), tested=int(cut["tested"][0]), accepted=int(cut["accepted"][0]))
    return out


@functools.lru_cache(maxsize=None)
def oracle_hit(name):
    """oracle.success_oracle.success_rows on the case's constant row: does it collide (at waypoint 0)"""
    c = next(c for c in LINK if c["name"] == name)
    res = SO.success_rows(OI.constant_row(c["q"])[None], np.asarray(c["oc"])[None], 1, np.array([c["kind"]], dtype=np.int32), OI.EXTENTS)
    assert res["within"][0] and res["first"][0] in (-1, 0)
    return bool(res["first"][0] == 0)


def wrong(cases, results, keys):
    """the cases whose result differs in one of `keys` from the class's truth, which is the oracle's too"""
    bad = []
    for c in cases:
        assert oracle_hit(c["name"]) == c["hit"], c["name"]
        want = dict(first=0 if c["hit"] else -1, ok=not c["hit"], tested=1, accepted=0 if c["hit"] else 1)
        got = results[c["name"]]
        if any(got[k] != want[k] for k in keys):
            bad.append((c["name"], {k: got[k] for k in keys}))
    return bad


def per_class(cases, bad):
    """class -> [cases, wrong]"""
    names = {b[0] if isinstance(b, tuple) else b for b in bad}
    out = {}
    for c in cases:
        n = out.setdefault(c["cls"], [0, 0])
        n[0] += 1
        n[1] += c["name"] in names
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_success_rows_in_scene_batches(batch_results, family):
    """first and ok of the constant row equal the class's truth and the oracle's"""
    cases = [c for c in LINK if c["family"] == family]
    bad = wrong(cases, batch_results, ("first", "ok"))
    record(test="success, scene batches", family=family, cases=len(cases), hits=sum(c["hit"] for c in cases), wrong=len(bad), classes=per_class(cases, bad))
    assert not bad, bad


@pytest.mark.parametrize("family", FAMILIES)
def test_shortcut_rows_in_scene_batches(batch_results, family):
    """the one candidate is tested, and accepted exactly when the class says miss"""
    cases = [c for c in LINK if c["family"] == family]
    bad = wrong(cases, batch_results, ("tested", "accepted"))
    record(test="shortcut, scene batches", family=family, cases=len(cases), hits=sum(c["hit"] for c in cases), wrong=len(bad), classes=per_class(cases, bad))
    assert not bad, bad


@pytest.mark.parametrize("family", FAMILIES)
def test_single_scene_guides(single_results, family):
    cases = [c for c in singles() if c["family"] == family]
    bad = wrong(cases, single_results, ("first", "ok", "tested", "accepted"))
    record(test="success and shortcut, single scenes", family=family, cases=len(cases), hits=sum(c["hit"] for c in cases), wrong=len(bad), classes=per_class(cases, bad))
    assert cases and not bad, bad


@pytest.fixture(scope="module")
def self_guide():
    return make_guide(LINK[0])


@pytest.mark.parametrize("family", SELF_FAMILIES)
def test_self_collision_rows_with_the_pair_alone(self_guide, family):
    """the constant row under a mask of the one pair: first and pair as the class says"""
    cases = [c for c in SELF if c["family"] == family]
    bad = []
    for c in cases:
        a, b = c["pair"]
        mask = np.zeros((9, 9), dtype=np.int32)
        mask[a, b] = 1
        res = self_guide.self_collision_rows(OI.constant_row(c["q"])[None], substeps=1, pairs=mask)
        got = (int(res["first"][0]), res["pair"][0].tolist(), bool(res["free"][0]))
        if got != ((0, [a, b], False) if c["hit"] else (-1, [-1, -1], True)):
            bad.append((c["name"], got))
    record(test="self-collision, one pair", family=family, cases=len(cases), hits=sum(c["hit"] for c in cases), wrong=len(bad), classes=per_class(cases, bad))
    assert cases and not bad, bad


def test_self_collision_rows_with_the_default_mask(self_guide):
    """the same rows in one call under the default mask, against the NumPy reference (which asserts that none of their masked pairs sits
    within 1e-9 m of its decision)"""
    X = np.stack([OI.constant_row(c["q"]) for c in SELF])
    ref = SCI.reference(X, 1)
    res = self_guide.self_collision_rows(X, substeps=1)
    bad = [c["name"] for r, c in enumerate(SELF) if res["first"][r] != ref["first"][r] or res["pair"][r].tolist() != ref["pair"][r].tolist() or res["free"][r] != ref["free"][r]]
    record(test="self-collision, default mask", cases=len(SELF), colliding=int((~ref["free"]).sum()), wrong=len(bad), classes=per_class(SELF, bad))
    assert not bad, bad
