#!/usr/bin/env python
"""Writes tests/golden/bf3_parent_bits.npz: what the PARENT commit's library computes for the forwards of tests/bf3_bits_inputs.py,
for tests/test_gpu_bf3_bits.py to hold a change to the bodies of the bf16x3 kernels (csrc/bf3.hip) to, bit for bit.

The forwards are defined in THIS checkout (tests/bf3_bits_inputs.py); the package that runs them comes from --tree: a worktree of the
parent commit, built there (python __graft_entry__.py), or any directory that holds that build's edmp_amd/ package.  Needs a GPU.

  git worktree add ../parent HEAD~1 && (cd ../parent && python __graft_entry__.py)
  python scripts/record_bf3_parent_bits.py --tree ../parent --commit $(git -C ../parent rev-parse HEAD)
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", required=True, help="directory whose edmp_amd/ package (with its built libraries) is the parent commit's")
    ap.add_argument("--commit", required=True, help="id of the parent commit, recorded in the file")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bf3_parent_bits.npz"))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    if not os.path.exists(os.path.join(tree, "edmp_amd", "libedmp_hip.so")):
        raise SystemExit(f"{tree}/edmp_amd/libedmp_hip.so not found: build the parent commit there first")
    sys.path.insert(0, tree)
    import edmp_amd

    if os.path.dirname(os.path.abspath(edmp_amd.__file__)) != os.path.join(tree, "edmp_amd"):
        raise SystemExit(f"edmp_amd was imported from {edmp_amd.__file__}, not from --tree")
    spec = importlib.util.spec_from_file_location("bf3_bits_inputs", os.path.join(ROOT, "tests", "bf3_bits_inputs.py"))
    I = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(I)
    out = {"parent_commit": np.array(args.commit), "B": np.array(I.B), "t": np.array(I.T_STEP), "rows": np.array(I.ROWS)}
    for name in I.ARCHS:
        rec = I.record(name)
        ops = [str(s) for s in rec[f"{name}_ops"]]
        want = I.BF3_FULL if name == "full" else I.BF3_SMALL
        missing = [n for n in want if n not in ops]
        if missing:
            raise SystemExit(f"{name}: the parent's program does not launch {missing}")
        out.update(rec)
        print(f"[{name}] dims {I.ARCHS[name][0]}: {len(ops)} ops, taps {rec[f'{name}_taps'].tolist()}, eps sha256 {I.digest(rec[f'{name}_eps'])[:16]}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, parent commit {args.commit}")


if __name__ == "__main__":
    main()
