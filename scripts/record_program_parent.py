#!/usr/bin/env python
"""Writes tests/golden/unet_program_parent.json: what the PARENT commit's library decides when it builds the models of
tests/program_record.py, for tests/test_gpu_program_record.py to hold a change to the host side of the model build (csrc/unet.hip: the
architecture walk, the packer, the layer program) to, value for value.

The cells are defined in THIS checkout (tests/program_record.py); the package that builds them comes from --tree: a worktree of the
parent commit, built there (python __graft_entry__.py), or any directory that holds that build's edmp_amd/ package.  Needs a GPU.

  git worktree add ../parent HEAD~1 && (cd ../parent && python __graft_entry__.py)
  python scripts/record_program_parent.py --tree ../parent --commit $(git -C ../parent rev-parse HEAD)

The file keeps every distinct value once (tests/program_record.py, pack()): many cells of a small architecture are the same model, and
a program repeats few distinct ops."""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write(P, out, commit, by_cell):
    """one row, one entry per line: a change to the record shows as the lines it changes"""
    rec = P.pack(by_cell)
    assert P.unpack(rec) == by_cell
    dumps = lambda v: json.dumps(v, separators=(",", ":"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(f'{{"parent_commit":{dumps(commit)},"max_batch":{P.MAX_BATCH},\n"cells":{dumps(rec["cells"])},\n')
        f.write('"rows":[\n' + ",\n".join(dumps(r) for r in rec["rows"]) + '],\n')
        f.write('"entries":[\n' + ",\n".join(dumps(e) for e in rec["entries"]) + ']}\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", required=True, help="directory whose edmp_amd/ package (with its built libraries) is the parent commit's")
    ap.add_argument("--commit", required=True, help="id of the parent commit, recorded in the file")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    if not os.path.exists(os.path.join(tree, "edmp_amd", "libedmp_hip.so")):
        raise SystemExit(f"{tree}/edmp_amd/libedmp_hip.so not found: build the parent commit there first")
    sys.path.insert(0, tree)
    import edmp_amd

    if os.path.dirname(os.path.abspath(edmp_amd.__file__)) != os.path.join(tree, "edmp_amd"):
        raise SystemExit(f"edmp_amd was imported from {edmp_amd.__file__}, not from --tree")
    if ROOT not in sys.path:
        sys.path.append(ROOT)  # behind --tree: the package stays the parent's
    spec = importlib.util.spec_from_file_location("program_record", os.path.join(ROOT, "tests", "program_record.py"))
    P = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(P)
    out = args.out or P.RECORD
    by_cell = {}
    for aid, setting in P.cells():
        t0 = time.perf_counter()
        e = by_cell[f"{aid}/{setting}"] = json.loads(json.dumps(P.cell(aid, setting)))
        print(f"[{aid}/{setting}] " + (f"refused: {e['refused']}" if "refused" in e else
              f"{len(e['ops'])} ops, layout {e['layout']}, image {e['image_sha256'][:16]}") + f" ({time.perf_counter() - t0:.2f} s)", flush=True)
    write(P, out, args.commit, by_cell)
    size = os.path.getsize(out)
    print(f"wrote {out}: {len(by_cell)} cells, {size} bytes, parent commit {args.commit}")
    if size > 1 << 20:
        raise SystemExit("the record is larger than 1 MiB")


if __name__ == "__main__":
    main()
