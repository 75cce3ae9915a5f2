#!/usr/bin/env python
"""Writes tests/golden/bf3_forward_parent.json: shape and SHA-256 of what the PARENT commit's library computes for the forwards of
tests/bf3_forward_inputs.py, for tests/test_gpu_bf3_forward_bits.py to hold a change to the bodies of the bf16x3 kernels (csrc/bf3.hip)
to, bit for bit.

The forwards are defined in THIS checkout (tests/bf3_forward_inputs.py); the package that runs them comes from --tree: a worktree of the
parent commit, built there (python __graft_entry__.py), or any directory that holds that build's edmp_amd/ package.  Needs a GPU.

  git worktree add ../parent HEAD~1 && (cd ../parent && python __graft_entry__.py)
  python scripts/record_bf3_forward_parent.py --tree ../parent --commit $(git -C ../parent rev-parse HEAD)
"""
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
    if not os.path.exists(os.path.join(tree, "edmp_amd", "libedmp_hip.so")):
        raise SystemExit(f"{tree}/edmp_amd/libedmp_hip.so not found: build the parent commit there first")
    sys.path.insert(0, tree)
    import edmp_amd

    if os.path.dirname(os.path.abspath(edmp_amd.__file__)) != os.path.join(tree, "edmp_amd"):
        raise SystemExit(f"edmp_amd was imported from {edmp_amd.__file__}, not from --tree")
    if ROOT not in sys.path:
        sys.path.append(ROOT)  # behind --tree: the package stays the parent's, tests/ is this checkout's
    from tests import bf3_forward_inputs as I

    out = args.out or os.path.join(ROOT, "tests", "golden", I.RECORD_NAME)
    rec = {"parent_commit": args.commit, "max_batch": I.MAX_BATCH, **I.record()}
    for k, case in rec["cases"].items():
        print(f"[{k}] eps {case['eps']['shape']} sha256 {case['eps']['sha256'][:16]}, taps {sorted(n for n in case if n != 'eps')}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {os.path.getsize(out)} bytes, parent commit {args.commit}")


if __name__ == "__main__":
    main()
