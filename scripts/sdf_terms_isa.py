#!/usr/bin/env python
"""Compares the gfx950 machine code of the sdf.hip kernels of two builds and writes profiles/sdf_terms_isa.json: per kernel a hash of
its disassembled function in either build and the VGPR / SGPR / LDS / scratch figures of the code object's notes.

  python scripts/sdf_terms_isa.py --parent ../parent/edmp_amd/csrc/_obj --tree edmp_amd/csrc/_obj --commit $(git -C ../parent rev-parse HEAD)

Each directory holds the sdf.o that the build (__graft_entry__.py) compiled there.  Needs ROCm's LLVM tools, no GPU.  The hash is over
the instruction text and encoding of every line of the function, addresses left out; --dropped names kernels in which a device helper
was taken out again because it changed them (recorded as the file's "helpers_dropped")."""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def device_image(obj, tmp):
    """the gfx950 code object inside the offload bundle of a host object file"""
    fb = os.path.join(tmp, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(tmp, "copy.o")], check=True)
    data = open(fb, "rb").read()
    pos = data.find(MAGIC)
    (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
    p = pos + len(MAGIC) + 8
    for _ in range(n):
        off, size, tlen = struct.unpack_from("<QQQ", data, p)
        triple = data[p + 24:p + 24 + tlen].decode()
        p += 24 + tlen
        if triple.startswith("hip") and triple.endswith("gfx950"):
            co = os.path.join(tmp, "device.co")
            open(co, "wb").write(data[pos + off:pos + off + size])
            return co
    raise SystemExit(f"{obj}: no gfx950 image in its offload bundle")


def kernels_of(obj):
    """{kernel name: {"sha256": ..., "instructions": n, figures...}} of one sdf.o"""
    with tempfile.TemporaryDirectory() as tmp:
        co = device_image(obj, tmp)
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = code.setdefault(m.group(1), [])
        elif cur is not None and "//" in line:
            text, _, tail = line.partition("//")
            cur.append(text.strip() + " | " + tail.split(":", 1)[1].strip())  # (the address before the colon is left out)
    out, entries = {}, []
    for line in notes.splitlines():  # an entry of amdhsa.kernels starts at "  - .key:", its own keys sit at four columns
        if line.startswith("  - ."):
            entries.append({})
            line = "    " + line[4:]
        m = re.match(r"^    \.([a-z_]+):\s+(\S+)$", line)
        if m and entries:
            entries[-1][m.group(1)] = m.group(2)
    for e in entries:
        if e.get("name") in code:
            out[e["name"]] = {k: int(e[k]) for k in FIGURES if k in e}
    for k in out:
        out[k].update(sha256=hashlib.sha256("\n".join(code[k]).encode()).hexdigest(), instructions=len(code[k]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent", required=True, help="directory with the parent build's sdf.o")
    ap.add_argument("--tree", required=True, help="directory with this tree's sdf.o")
    ap.add_argument("--commit", default=None, help="id of the parent commit, recorded in the file")
    ap.add_argument("--dropped", nargs="*", default=[], help="kernels in which a device helper was taken out again")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_terms_isa.json"))
    args = ap.parse_args()
    a, b = kernels_of(os.path.join(args.parent, "sdf.o")), kernels_of(os.path.join(args.tree, "sdf.o"))
    rec = {"parent_commit": args.commit, "helpers_dropped": args.dropped, "kernels": {}}
    for k in sorted(set(a) | set(b)):
        pa, tr = a.get(k), b.get(k)
        rec["kernels"][k] = {"parent": pa, "tree": tr, "identical": pa == tr}
        print(f"{'same' if pa == tr else 'DIFFERENT':9s} {k}: parent {pa and (pa['instructions'], pa['vgpr_count'])}, tree {tr and (tr['instructions'], tr['vgpr_count'])}")
    rec["all_identical"] = all(v["identical"] for v in rec["kernels"].values())
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}: {len(rec['kernels'])} kernels, all identical: {rec['all_identical']}")
    return 0 if rec["all_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
