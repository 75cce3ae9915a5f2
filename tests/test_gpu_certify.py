"""The continuous certificate (certify_rows_kernel, edmp_certify_rows_dev, edmp_scenes_certify_rows_dev) on the GPU against the rule of
tests/certify_inputs.py on admitted cases, against the GPU's own success_rows as the judge, and against itself where the property is
bit-equality.

On an admitted case (no decision of the rule sits on a rounding) verdict, segment, link, evaluations, undecided and the dyadic fraction are
compared exactly, with the rule run on the radii table the library returns.  bound is compared under a gate of 4 x a yardstick PER CASE:
the largest deviation, over the case's rows, of the float64 rule from the same rule evaluated in numpy.longdouble - what the number type
itself costs on these inputs - with a floor of one ulp of the case's largest finite bound (no float64 result can be held closer than its
own rounding), and this project's margin of 4 (the kernel may contract to fused multiply-adds, so bit equality is not asked).  Every comparison prints its error, yardstick and gate; with EDMP_CERTIFY_PARITY_OUT=<file> the records are written there as JSON
(profiles/certify_parity.json comes from such a run)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from edmp_amd import franka
from tests import certify_inputs as I
from tests import repair_inputs as RI
from tests import stream_order as S
from tests.sdf_gpu import DEV, recorder, run_cfgs, tiny_net  # noqa: F401  (tiny_net: this module's fixture)
from tests.sdf_term_suite import segmented_run_goes_on

pytestmark = pytest.mark.gpu
record, _write_records = recorder("certify parity", "EDMP_CERTIFY_PARITY_OUT",
                                  "verdict, segment, link, evaluations, undecided and fraction exactly; bound within 4 x the case's own largest deviation of the "
                                  "float64 host rule from the numpy.longdouble host rule, floor one ulp of the case's largest finite bound")
GATE = 4.0


def yardstick(name):
    """the case's largest |bound(float64 rule) - bound(longdouble rule)|, at least one ulp of its largest finite bound"""
    case = I.case(name)
    b = case["ref"]["bound"]
    fin = np.isfinite(b)
    return max(case["deviation"], float(np.spacing(np.abs(b[fin]).max())) if fin.any() else 0.0)


def make_guide(case, device=DEV, **kw):
    """the guide of a case: its obstacles and kinds and the placeholder link boxes (certify_inputs.EXTENTS); the stage reads no row array"""
    from edmp_amd.guide import IntersectionVolumeGuide

    cfgs = case["cfgs"]
    return IntersectionVolumeGuide(case["obstacle_config"], device, cfgs, cfgs["total_batch_size"], link_mesh_extents=franka.PLACEHOLDER_LINK_EXTENTS,
                                   obstacle_kinds=case["kinds"], **kw)


def bits(a):
    """raw bits, NaN patterns included"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same(a, b, keys=I.KEYS):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def rule_on_the_library_radii(case, out):
    """the rule's result with the table the library returned: the case's own (computed once) where the two tables have the same bits"""
    if np.array_equal(out["radii"], franka.motion_radii(I.EXTENTS)):
        return case["ref"]
    return I.certify_rows(case["X"], case["obstacle_config"], case["kinds"], case["D"], case["margin"], rho=out["radii"])


def compare(name, out, ref, rows=None, test="rule"):
    """the exact keys exactly, bound within the gate, on `rows` (all) -> the bound's error"""
    rows = np.arange(len(ref["verdict"])) if rows is None else np.asarray(rows)
    y = yardstick(name)
    fin = np.isfinite(ref["bound"][rows])
    err = float(np.abs(out["bound"][rows][fin] - ref["bound"][rows][fin]).max()) if fin.any() else 0.0
    record(test=test, case=name, rows=rows.tolist(), verdict=out["verdict"][rows].tolist(), evaluations=out["evaluations"][rows].tolist(), bound_abs_err=err,
           case_deviation=I.case(name)["deviation"], yardstick=y, gate=GATE)
    for k in I.INT_KEYS:
        assert out[k].dtype == np.int32 and np.array_equal(out[k][rows], ref[k][rows]), (name, k, out[k][rows].tolist(), ref[k][rows].tolist())
    assert np.array_equal(bits(out["fraction"][rows]), bits(ref["fraction"][rows])), (name, out["fraction"][rows].tolist(), ref["fraction"][rows].tolist())
    assert np.array_equal(np.isfinite(out["bound"][rows]), fin) and (out["bound"][rows][~fin] == np.inf).all(), name
    assert err <= GATE * y, (name, err, y)
    return err


@pytest.mark.parametrize("name", list(I.CASES))
def test_against_the_rule(name):
    """every listed case: the integers and the fraction exactly, bound within 4 x the yardstick; the radii the library used are
    franka.motion_radii's to 1e-15 relative"""
    case = I.case(name)
    out = make_guide(case).certify_rows(case["X"], depth=case["D"], margin=case["margin"])
    want = franka.motion_radii(I.EXTENTS)
    assert out["radii"].shape == (9, 7) and np.all(np.abs(out["radii"] - want) <= 1e-15 * np.abs(want))
    assert (out["depth"], out["margin"]) == (case["D"], case["margin"])
    compare(name, out, rule_on_the_library_radii(case, out))


def test_row_counts_and_shuffled_subsets():
    """the 9-row case on its first 1 .. 9 rows, each against the rule; then shuffled row subsets: the listed rows equal their values from
    the all-rows call bit for bit, the others report verdict -1 and a NaN bound; the same row at another index gives the same bits"""
    name = "N14_o5_n9"
    case = I.case(name)
    guide = make_guide(case)
    kw = dict(depth=case["D"], margin=case["margin"])
    full = guide.certify_rows(case["X"], **kw)
    ref = rule_on_the_library_radii(case, full)
    for n in range(1, 10):
        out = make_guide(dict(case, cfgs=RI.plain_cfgs(n))).certify_rows(case["X"][:n], **kw)
        compare(name, out, ref, rows=np.arange(n), test=f"first {n} rows")
    rs = np.random.RandomState(3)
    for n in (1, 4, 9):
        listed = rs.permutation(9)[:n]
        part = guide.certify_rows(case["X"], rows=listed.tolist(), **kw)
        rest = np.setdiff1d(np.arange(9), listed)
        for k in I.KEYS:
            assert np.array_equal(bits(part[k][listed]), bits(full[k][listed])), (n, k)
        assert (part["verdict"][rest] == -1).all() and (part["segment"][rest] == -1).all() and (part["link"][rest] == -1).all()
        assert (part["evaluations"][rest] == 0).all() and (part["undecided"][rest] == 0).all() and (part["fraction"][rest] == -1.0).all() and np.isnan(part["bound"][rest]).all()
    perm = rs.permutation(9)
    moved = guide.certify_rows(np.ascontiguousarray(case["X"][perm]), **kw)
    assert all(np.array_equal(bits(moved[k]), bits(full[k][perm])) for k in I.KEYS)
    assert len(set(full["verdict"].tolist())) == 3  # (free, hit and undecided rows among the nine)


def test_free_rows_pass_the_sampled_check_on_the_gpu():
    """every row the GPU certifies free passes the GPU's own success_rows at 1, 4, 7 and 64 substeps, boxes and cylinders"""
    seen = 0
    for name in ("N9_o7c2_n3_D1", "N14_o7c2_n5_margin", "N14_o5_n9", "N3_graze_free_D4", "N5_special"):
        case = I.case(name)
        guide = make_guide(case)
        out = guide.certify_rows(case["X"], depth=case["D"], margin=case["margin"])
        free = out["verdict"] == 0
        assert np.array_equal(free, case["ref"]["verdict"] == 0) and free.any(), name
        for K in (1, 4, 7, 64):
            chk = guide.success_rows(case["X"], substeps=K)
            assert (chk["first"][free] == -1).all() and chk["collision_free"][free].all(), (name, K)
        assert (out["bound"][free] > case["margin"]).all()
        seen += int(free.sum())
    assert seen >= 10


@pytest.mark.parametrize("name", ["plate_box", "plate_cylinder", "plate_box_D10"])
def test_tunnelling_on_the_gpu(name):
    """a thin plate between the configurations the sampled check tests: success_rows at 4 substeps calls the row free, certify_rows reports
    the hit the rule names"""
    case = I.case(name)
    guide = make_guide(case)
    chk = guide.success_rows(case["X"], substeps=4)
    assert chk["first"][0] == -1 and chk["collision_free"][0]
    out = guide.certify_rows(case["X"], depth=case["D"])
    ref = case["ref"]
    assert out["verdict"][0] == 1 and (out["segment"][0], out["fraction"][0], out["link"][0]) == (ref["segment"][0], ref["fraction"][0], ref["link"][0])
    assert guide.success_rows(case["X"], substeps=64)["first"][0] >= 0


def test_scene_batch_equals_serial_runs():
    """two scenes with 7 (2 cylinders) and 3 obstacles, 3 rows each: every output of scene s equals guides[s].certify_rows(X[s]) bit for
    bit, also with the scenes in reversed order, with the state and the results on the device, and on a row subset"""
    from edmp_amd.guide import SceneBatch

    parts = [dict(I.smooth_rows(2, 3, 9, 7, 2), cfgs=RI.plain_cfgs(3)), dict(I.smooth_rows(3, 3, 9, 3, 0), cfgs=RI.plain_cfgs(3))]
    kw = dict(depth=5, margin=0.01)
    for order in ((0, 1), (1, 0)):
        ps = [parts[i] for i in order]
        guides = [make_guide(p) for p in ps]
        serial = [g.certify_rows(p["X"], **kw) for g, p in zip(guides, ps)]
        batch = SceneBatch(guides)
        X = np.stack([p["X"] for p in ps])
        got = batch.certify_rows(X, **kw)
        assert got["verdict"].shape == (2, 3) and got["bound"].shape == (2, 3) and got["radii"].shape == (9, 7)
        for s in range(2):
            for k in I.KEYS:
                assert np.array_equal(bits(got[k][s]), bits(serial[s][k])), (order, s, k)
        assert not same(serial[0], serial[1]) and all((o["evaluations"] > 0).all() for o in serial)
        cpu = batch.certify_rows(torch.as_tensor(X), **kw)  # (a CPU tensor is a host array)
        assert all(isinstance(cpu[k], np.ndarray) and np.array_equal(bits(cpu[k]), bits(got[k])) for k in I.KEYS)
        Xd = torch.as_tensor(X, device=DEV)
        for obj, state in ((batch, Xd), (guides[1], Xd[1])):  # the Python calls are host-only: a device tensor is refused, not copied behind the caller's back
            with pytest.raises(TypeError, match="host arrays"):
                obj.certify_rows(state, **kw)
        sub = batch.certify_rows(X, rows=[5, 0], **kw)  # (rows index the S*B rows scene after scene)
        for k in I.KEYS:
            assert np.array_equal(bits(sub[k][1, 2]), bits(got[k][1, 2])) and np.array_equal(bits(sub[k][0, 0]), bits(got[k][0, 0])), k
        assert (sub["verdict"].reshape(-1)[[1, 2, 3, 4]] == -1).all()


def test_a_segmented_run_goes_on(tiny_net):
    """a certify_rows call between two segments of a segmented run: the run's result is bit-identical to the uninterrupted one"""
    from edmp_amd import scenes
    from edmp_amd.guide import IntersectionVolumeGuide
    from tests import shortcut_inputs as SI

    cfgs = run_cfgs(101)
    s, gl = np.asarray(scenes.DEFAULT_START, dtype=np.float64), np.asarray(scenes.DEFAULT_GOAL, dtype=np.float64)
    rs = np.random.RandomState(11)
    g = IntersectionVolumeGuide(scenes.random_scene(7, 8), DEV, cfgs, cfgs["total_batch_size"])

    def between():  # (called once, after the noise of both segments has been drawn from rs)
        return g.certify_rows(SI.zigzag_rows(gl, s, 50, 5), depth=4, rows=[4, 1])

    mid = segmented_run_goes_on(tiny_net, g, cfgs, s, gl, rs, between)
    assert (mid["verdict"][[4, 1]] >= 0).all() and (mid["evaluations"][[4, 1]] >= 49 * 9).all() and mid["verdict"][0] == -1


def raw_call(guide, Xd, rows=None, n=None, N=None, depth=4, margin=0.0, name="edmp_certify_rows_dev", lead=None, null=None):
    """the C entry point on a device state, with result buffers that a refused call must leave as they are -> (rc, message, ints, reals, radii)"""
    from edmp_amd import _capi
    from edmp_amd.runtime import ptr

    ctx = guide.ctx
    n = Xd.shape[0] if n is None else n
    with torch.cuda.stream(ctx.stream):
        ints = torch.full((5, Xd.shape[0]), -7, dtype=torch.int32, device=ctx.device)
        reals = torch.full((2, Xd.shape[0]), -5.0, dtype=torch.float64, device=ctx.device)
    lst = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32))
    lead = (n,) if lead is None else lead
    dh = np.ascontiguousarray(franka.dh_table_f64())
    radii = np.full(63, -3.0)
    outs = [C.c_void_p(ints[0].data_ptr()), C.c_void_p(ints[1].data_ptr()), C.c_void_p(reals[0].data_ptr()), C.c_void_p(ints[2].data_ptr()), C.c_void_p(ints[3].data_ptr()),
            C.c_void_p(ints[4].data_ptr()), C.c_void_p(reals[1].data_ptr())]
    if null is not None:
        outs[null] = None
    rc = getattr(ctx.lib, name)(ctx.h, ptr(Xd), *lead, Xd.shape[2] if N is None else N, None if lst is None else _capi.as_pi32(lst), 0 if lst is None else len(lst),
                                depth, margin, _capi.as_pd(dh), *outs, _capi.as_pd(radii))
    return rc, (ctx.lib.edmp_last_error() or b"").decode() if rc else "", ctx.to_host(ints), ctx.to_host(reals), radii


def test_stream_ordering():
    """a call ordered after a pending producer sees its data.  The entry points run on the context's stream and the Python calls take host
    arrays only, so the producer a caller can have pending is one on that stream: the device state made late behind a hold
    (tests/stream_order.py: poison until the hold in front of its copy ends) gives the bits of the call on a state that has landed.  An
    attempt decides only if the hold was still running when the call was made"""
    case = I.case("N14_o7c2_n5_margin")
    S.calibration()  # (the hold's calibration runs the table's calls on this context and binds their objects: before this test's guide is bound, not inside late())
    guide = make_guide(case)
    guide._bind()
    ctx = guide.ctx
    good = S.ready(case["X"], ctx.device)
    rc, msg, want_i, want_r, _ = raw_call(guide, good, depth=case["D"], margin=case["margin"])
    assert rc == 0 and np.array_equal(want_i[0], case["ref"]["verdict"]), msg
    decided = False
    for _ in range(S.ATTEMPTS):
        late = S.late(good, ctx.stream)
        running = not S._state["late_behind"].query()
        rc, msg, got_i, got_r, _ = raw_call(guide, late, depth=case["D"], margin=case["margin"])
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(got_i, want_i) and np.array_equal(bits(got_r), bits(want_r)), msg
        if running:
            decided = True
            break
    assert decided, "the hold had always ended before the call was made: nothing was decided"


def test_refusals():
    """each bad argument, duplicate rows included, is refused with a message that names the entry point and the argument; the result
    buffers and a following call are what they were"""
    from edmp_amd import _capi
    from edmp_amd.guide import SceneBatch

    case = I.case("N14_o7c2_n5_margin")
    guide = make_guide(case)
    before = guide.certify_rows(case["X"], depth=4)
    Xd = guide.ctx.to_dev(case["X"], torch.float64)
    bad = (("N = 1", dict(N=1), "(got 1)"), ("N = 65", dict(N=65), "(got 65)"), ("depth = -1", dict(depth=-1), "depth -1"), ("depth = 11", dict(depth=11), "depth 11"),
           ("negative margin", dict(margin=-0.5), "margin -0.5"), ("NaN margin", dict(margin=float("nan")), "margin"), ("inf margin", dict(margin=float("inf")), "margin inf"),
           ("row 5 of 5", dict(rows=[0, 5]), "rows[1] = 5"), ("row -1", dict(rows=[-1]), "rows[0] = -1"), ("a row twice", dict(rows=[1, 0, 1]), "rows[2] = 1 is listed twice"),
           ("more rows than there are", dict(rows=[0, 1, 2, 3, 4, 0]), "6 listed rows"), ("n = 0", dict(n=0), "n >= 1"), ("a null output", dict(null=6), "null pointer"))
    for what, kw, needle in bad:
        rc, msg, ints, reals, radii = raw_call(guide, Xd, **kw)
        assert rc == -1 and msg.startswith("edmp_certify_rows_dev") and needle in msg, (what, rc, msg)
        assert (ints == -7).all() and (reals == -5.0).all() and (radii == -3.0).all(), what
    rc, msg, ints, _, _ = raw_call(guide, Xd, name="edmp_scenes_certify_rows_dev", lead=(1, 5))  # the batch's entry point on a single-scene guide
    assert rc == -3 and msg.startswith("edmp_scenes_certify_rows_dev") and (ints == -7).all(), (rc, msg)
    assert np.array_equal(bits(guide.ctx.to_host(Xd)), bits(case["X"]))
    assert same(guide.certify_rows(case["X"], depth=4), before)
    # the accepted raw call writes the listed rows only, and the radii
    rc, msg, ints, reals, radii = raw_call(guide, Xd, rows=[2])
    assert rc == 0, msg
    assert ints[:, 2].tolist() == [before[k][2] for k in I.INT_KEYS] and (ints[:, [0, 1, 3, 4]] == -7).all() and (reals[:, [0, 1, 3, 4]] == -5.0).all()
    assert reals[:, 2].tolist() == [before["fraction"][2], before["bound"][2]] and np.array_equal(radii.reshape(9, 7), before["radii"])
    with pytest.raises(ValueError):
        guide.certify_rows(np.zeros((3, 6, 4)))
    with pytest.raises(_capi.EdmpError, match="depth 12"):
        guide.certify_rows(case["X"], depth=12)
    # the single-scene entry point on a bound batch of two scenes, and a batch call with the wrong scene count
    batch = SceneBatch([make_guide(case, bind=False), make_guide(case, bind=False)])
    batch._bind()
    X2 = batch.ctx.to_dev(np.concatenate([case["X"], case["X"]]), torch.float64)
    rc, msg, _, _, _ = raw_call(batch, X2)
    assert rc == -3 and msg.startswith("edmp_certify_rows_dev"), (rc, msg)
    rc, msg, _, _, _ = raw_call(batch, X2, name="edmp_scenes_certify_rows_dev", lead=(3, 5))
    assert rc == -1 and msg.startswith("edmp_scenes_certify_rows_dev"), (rc, msg)
    with pytest.raises(_capi.EdmpError, match="listed twice"):
        batch.certify_rows(np.stack([case["X"], case["X"]]), rows=[4, 4])


def test_driver_certifies_between_the_shortcuts_and_the_selection(capsys):
    """infer_serial --certify on the driver test's two seeded scenes: off, no key is added and nothing is printed of it; on, the serial loop
    and the scene-group path (one launch) report the same census, and the chosen plan is the run's without the option"""
    import infer_serial
    from edmp_amd import scenes

    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "cfg_c1_plumbing.yaml")

    def run(k, certify, verbose=False):
        np.random.seed(31)
        ds = scenes.SyntheticDataset(scene_types=("stress",), num_scenes_per_type=2, n_obstacles=6, n_cylinders=1)
        return infer_serial.run(cfg, dataset=ds, verbose=verbose, scenes_per_launch=k, certify=certify, certify_margin=0.005)

    off = run(1, None, verbose=True)
    printed_off = capsys.readouterr().out
    serial = run(1, 4, verbose=True)
    printed_on = capsys.readouterr().out
    group = run(2, 4)
    assert len(off) == len(serial) == len(group) == 2
    assert "certificate" not in printed_off and printed_on.count("    certificate (depth 4, margin 0.005 m): rows free ") == 2
    strip = lambda text: [ln for ln in text.splitlines() if "certificate" not in ln and "planning" not in ln]  # noqa: E731  (the planning line carries a time)
    assert strip(printed_on) == strip(printed_off)
    for o, a, b in zip(off, serial, group):
        assert not any(k.startswith("certify") or k == "rows_passed_but_certified_hit" for k in o) and "certify_s" not in o["timings"]
        assert "certify_s" in a["timings"] and "certify_s" in b["timings"]
        for k in ("certify_rows", "rows_passed_but_certified_hit", "certify_verdict", "certify_depth", "certify_margin", "best_row"):
            assert a[k] == b[k], k
        assert a.get("certify_bound") == b.get("certify_bound") and a.get("certify_at") == b.get("certify_at")
        assert sum(a["certify_rows"].values()) == a["rows"] and a["certify_rows"]["invalid"] == 0 and a["certify_depth"] == 4
        assert 0 <= a["rows_passed_but_certified_hit"] <= a["rows_collision_free"]
        assert a["certify_rows"]["free"] <= a["rows_collision_free"]  # (a certified row passes the sampled check)
        assert ("certify_bound" in a) == (a["certify_verdict"] == "free") and ("certify_at" in a) == (a["certify_verdict"] in ("hit", "undecided"))
        assert (o["best_row"], o["success_proxy"]) == (a["best_row"], a["success_proxy"]) and np.array_equal(o["trajectory"], a["trajectory"])
    for bad in (-1, 11):
        with pytest.raises(ValueError):
            infer_serial.run(cfg, verbose=False, certify=bad)
