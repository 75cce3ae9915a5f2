#!/usr/bin/env python
"""Writes tests/golden/sampler_parent.json: what the PARENT commit's Diffusion.denoise_guided / denoise_guided_scenes return, draw and ask
of the library for the cells of tests/sampler_cells.py, for tests/test_gpu_sampler_record.py to hold a restructuring of the two methods
to, with equality.  Needs a GPU.

The cells are defined in THIS checkout; the package that evaluates them comes from --tree: a directory that holds the parent commit's
built edmp_amd/ and no tests/ package (tests/ must stay this checkout's).

  git worktree add ../parent HEAD~1 && (cd ../parent && python __graft_entry__.py)
  mkdir ../parent_build && cp -r ../parent/edmp_amd ../parent_build/
  python scripts/record_sampler_parent.py --tree ../parent_build --commit $(git -C ../parent rev-parse HEAD)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", required=True, help="directory whose edmp_amd/ package (with its built libraries) is the parent commit's")
    ap.add_argument("--commit", required=True, help="id of the parent commit, recorded in the file")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import edmp_amd

    if os.path.abspath(edmp_amd.__file__) != os.path.join(tree, "edmp_amd", "__init__.py"):
        raise SystemExit(f"edmp_amd was imported from {edmp_amd.__file__}, not from --tree")
    sys.path.append(ROOT)  # behind --tree: the package stays the parent's, tests/ is this checkout's
    import tests

    if os.path.dirname(os.path.abspath(tests.__file__)) != os.path.join(ROOT, "tests"):
        raise SystemExit(f"tests was imported from {tests.__file__}, not from this checkout: --tree must not hold a tests/ package")
    from tests import sampler_cells as cells

    out = args.out or cells.RECORD
    rec = {"parent_commit": args.commit, "cells": {}}
    for name in cells.cell_names():
        c = rec["cells"][name] = cells.evaluate(name)
        print(f"{name}: {c['error'] if 'error' in c else [r['sha'][:12] for r in c['results']]}, {sum(n for _, n in c['calls']['base'])} calls", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:  # one cell per line, in the order of their names
        names = sorted(rec["cells"])
        f.write('{"parent_commit": %s,\n"cells": {\n' % json.dumps(args.commit))
        for k, name in enumerate(names):
            f.write(json.dumps(name) + ": " + json.dumps(rec["cells"][name], sort_keys=True, separators=(",", ":")) + (",\n" if k < len(names) - 1 else "\n"))
        f.write("}}\n")
    size = os.path.getsize(out)
    print(f"wrote {out}: {len(rec['cells'])} cells, {size} bytes, parent commit {args.commit}")
    if size > 1 << 20:
        raise SystemExit("the record is larger than 1 MiB")


if __name__ == "__main__":
    main()
