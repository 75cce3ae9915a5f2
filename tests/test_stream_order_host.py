"""tests/stream_order.TABLE against the package, by `inspect`, on the CPU: an entry point that takes or returns device tensors and has no
record - so that no GPU test holds its stream order - fails here."""
import importlib
import inspect
import re

from tests import stream_order as S

MODULES = ("guide", "evaluation", "diffusion", "ik", "temporalunet")
TOUCHES_DEVICE_INPUT = re.compile(r"adopt\(|\.is_cuda|_rows_f64\(|_rows_state\(|_device_f64\(")


def functions():
    """{module.qualname: function} of every function and method defined in MODULES (a class's own members only: an inherited worker counts
    where it is defined)"""
    out = {}
    for m in MODULES:
        mod = importlib.import_module(f"edmp_amd.{m}")
        for name, obj in vars(mod).items():
            if inspect.isfunction(obj) and obj.__module__ == mod.__name__:
                out[f"{m}.{name}"] = obj
            elif inspect.isclass(obj) and obj.__module__ == mod.__name__:
                for k, v in vars(obj).items():
                    if inspect.isfunction(v):
                        out[f"{m}.{name}.{k}"] = v
    return out


def public(qualname):
    return not any(part.startswith("_") for part in qualname.split(".")[1:])


def missing_records(table):
    """(public callables with a return_device parameter and no return_device record, functions that touch a caller's device tensor and are
    neither a record's target nor in any record's covers)"""
    fns = functions()
    with_rd = {e.target for e in table if e.return_device}
    named = {e.target for e in table} | {c for e in table for c in e.covers}
    a = sorted(q for q, f in fns.items() if public(q) and "return_device" in inspect.signature(f).parameters and q not in with_rd)
    b = sorted(q for q, f in fns.items() if TOUCHES_DEVICE_INPUT.search(inspect.getsource(f)) and q not in named)
    return a, b


def test_every_entry_point_has_a_record():
    no_record, uncovered = missing_records(S.TABLE)
    assert not no_record, f"public callables with return_device and no record in tests/stream_order.TABLE: {no_record}"
    assert not uncovered, f"functions that adopt or test a caller's device tensor and that no record names in its covers: {uncovered}"


def test_the_table_names_what_exists():
    """every target and every cover is a function of the package, every name is used once, and a record's device arguments and results are
    stated (an entry without either has nothing to order)"""
    fns = functions()
    for e in S.TABLE:
        assert e.target in fns and public(e.target), e.target
        for c in e.covers:
            assert c in fns, (e.name, c)
        assert e.device_args or e.device_results, e.name
        if e.return_device:
            assert "return_device" in inspect.signature(fns[e.target]).parameters, e.name
    assert len({e.name for e in S.TABLE}) == len(S.TABLE)
    lane = [e.name for e in S.TABLE if e.in_flight]
    assert lane and all(S.BY_NAME[n].return_device for n in lane)


def test_a_removed_record_is_noticed():
    """without the record of SceneBatch.time_rows the first check names that method; without every record that covers _device_f64 the
    second check names that helper"""
    cut = tuple(e for e in S.TABLE if e.name != "scenes_time_rows")
    assert missing_records(cut)[0] == ["guide.SceneBatch.time_rows"]
    cut = tuple(e for e in S.TABLE if "evaluation._device_f64" not in e.covers)
    assert "evaluation._device_f64" in missing_records(cut)[1]
