#!/usr/bin/env python
"""Writes tests/golden/driver_parent.json: what the PARENT commit's infer_serial.run returns, prints and asks of the library for the cells
of tests/driver_cells.py, for tests/test_gpu_driver_record.py to hold a restructuring of the driver to, with equality.  Needs a GPU.

The cells are defined in THIS checkout; infer_serial.py and the package that evaluate them come from --tree: a directory that holds the
parent commit's infer_serial.py and its built edmp_amd/ and no tests/ package (tests/ must stay this checkout's).

  git worktree add ../parent HEAD~1 && (cd ../parent && python __graft_entry__.py)
  mkdir ../parent_build && cp -r ../parent/infer_serial.py ../parent/edmp_amd ../parent_build/
  python scripts/record_driver_parent.py --tree ../parent_build --commit $(git -C ../parent rev-parse HEAD)"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", required=True, help="directory whose infer_serial.py and edmp_amd/ package (with its built libraries) are the parent commit's")
    ap.add_argument("--commit", required=True, help="id of the parent commit, recorded in the file")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import edmp_amd
    import infer_serial

    for mod, want in ((edmp_amd, os.path.join(tree, "edmp_amd", "__init__.py")), (infer_serial, os.path.join(tree, "infer_serial.py"))):
        if os.path.abspath(mod.__file__) != want:
            raise SystemExit(f"{mod.__name__} was imported from {mod.__file__}, not from --tree")
    sys.path.append(ROOT)  # behind --tree: the driver and the package stay the parent's, tests/ is this checkout's
    import tests

    if os.path.dirname(os.path.abspath(tests.__file__)) != os.path.join(ROOT, "tests"):
        raise SystemExit(f"tests was imported from {tests.__file__}, not from this checkout: --tree must not hold a tests/ package")
    from tests import driver_cells as cells

    out = args.out or cells.RECORD
    rec = {"parent_commit": args.commit, "cells": {}}
    for name in cells.CELLS:
        with tempfile.TemporaryDirectory() as tmp:
            rec["cells"][name] = cells.evaluate(name, tmp)
        print(f"{name}: {len(rec['cells'][name]['scenes'])} scenes, {len(rec['cells'][name]['printed'])} lines", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    size = os.path.getsize(out)
    print(f"wrote {out}: {len(rec['cells'])} cells, {size} bytes, parent commit {args.commit}")
    if size > 1 << 20:
        raise SystemExit("the record is larger than 1 MiB")


if __name__ == "__main__":
    main()
