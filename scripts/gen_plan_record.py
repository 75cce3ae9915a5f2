"""Writes tests/golden/unet_plan_record.json: per (architecture, builder-switch setting) of tests/plan_record.py the layout id, the
image size and the kernel instances of the dry layer plan (edmp_unet_plan_describe; no GPU).  The record pins which instance every
model picks: regenerate it only with a change that means to move that choice, never to make a refactor of the selection code pass."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import plan_record as R  # noqa: E402

names, plans, cells = [], [], {}  # each kernel name and each (counts, sha256) once; a cell is [layout, n_packed, index into plans]
for aname, arch in R.archs().items():
    for sname, setting in R.SETTINGS.items():
        d = R.describe(arch, setting)
        names += [k for k in d["counts"] if k not in names]
        p = {"counts": [[names.index(k), c] for k, c in d["counts"].items()], "sha256": d["sha256"]}
        if p not in plans:
            plans.append(p)
        cells.setdefault(aname, {})[sname] = [d["layout"], d["n_packed"], plans.index(p)]
with open(R.RECORD, "w") as f:
    json.dump({"names": names, "plans": plans, "cells": cells}, f, separators=(",", ":"), sort_keys=True)
    f.write("\n")
print(f"{R.RECORD}: {sum(len(c) for c in cells.values())} cells, {len(plans)} distinct plans, {os.path.getsize(R.RECORD)} bytes")
