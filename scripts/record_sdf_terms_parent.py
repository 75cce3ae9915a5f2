#!/usr/bin/env python
"""Writes tests/golden/sdf_terms_parent.json: what the PARENT commit's package gives for the cells of tests/sdf_terms_cells.py - the
digests of the row arrays and host tables of the SDF guide's optional terms, the verdicts on odd inputs, and (with --gpu) the
gradients, reports and refusal texts of the library - for tests/test_sdf_terms_host.py and tests/test_gpu_sdf_terms.py to hold a
change to that host path to, bit for bit.

The cells are defined in THIS checkout; the package that evaluates them comes from --tree: a worktree of the parent commit, built
there (python __graft_entry__.py), or any directory that holds that build's edmp_amd/ package.

  git worktree add ../parent HEAD~1 && (cd ../parent && python __graft_entry__.py)
  python scripts/record_sdf_terms_parent.py --tree ../parent --commit $(git -C ../parent rev-parse HEAD) [--gpu]

Without --gpu the "gpu" part of an existing record is kept as it is, and the other way round with --gpu-only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", required=True, help="directory whose edmp_amd/ package (with its built libraries) is the parent commit's")
    ap.add_argument("--commit", required=True, help="id of the parent commit, recorded in the file")
    ap.add_argument("--gpu", action="store_true", help="record the GPU cells too")
    ap.add_argument("--gpu-only", action="store_true", help="record the GPU cells and keep the host part of the existing record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import edmp_amd

    if os.path.dirname(os.path.abspath(edmp_amd.__file__)) != os.path.join(tree, "edmp_amd"):
        raise SystemExit(f"edmp_amd was imported from {edmp_amd.__file__}, not from --tree")
    sys.path.append(ROOT)  # behind --tree: the package stays the parent's, tests/ is this checkout's
    import tests

    if os.path.dirname(os.path.abspath(tests.__file__)) != os.path.join(ROOT, "tests"):
        raise SystemExit(f"tests was imported from {tests.__file__}, not from this checkout: --tree must not hold a tests/ package")
    from tests import sdf_terms_cells as cells

    out = args.out or cells.RECORD
    rec = json.load(open(out)) if os.path.exists(out) else {}
    rec["parent_commit"] = args.commit
    if not args.gpu_only:
        rec["host"] = cells.host_record()
    if args.gpu or args.gpu_only:
        rec["gpu"] = cells.gpu_record()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    size = os.path.getsize(out)
    print(f"wrote {out}: {', '.join(f'{k}: {len(v)}' for k, v in rec.items() if isinstance(v, dict))}, {size} bytes, parent commit {args.commit}")
    if size > 1 << 20:
        raise SystemExit("the record is larger than 1 MiB")


if __name__ == "__main__":
    main()
