"""Resource contract of the built library (CPU): the gfx950 code objects in libedmp_hip.so's .hip_fatbin, read with
llvm-readelf --notes.

* CU claim of the bf16x3 kernels (bf3.hip: bf3_conv_kernel).  A bf16x3 workgroup must own its CU: its eight waves (two per SIMD) claim
  256 VGPRs each, the whole 512-entry file, so that no wave of another kernel lands beside it.  That is the only containment of the
  open co-residency fault in profiles/r06_coresidency_fault.md, and it rests on an `asm volatile("v_mov_b32 v255, 0")`, on the
  launch bounds and on the launch size: a compiler update, an edit of either, or a new instance without the line loses it silently.
* every instance the layer program can launch (kernel_instances.h) is in the library exactly once;
* no kernel uses scratch (private segment, VGPR spills), with one documented allowance.
"""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edmp_amd", "csrc")
LIB = os.path.join(ROOT, "edmp_amd", "libedmp_hip.so")
LLVM = "/opt/rocm/llvm/bin"

VGPR_FILE = 512  # VGPR + AGPR entries per lane per SIMD on gfx950 (one unified file)
VGPR_GRANULE = 8  # allocation granule, registers per lane
SIMDS_PER_CU = 4
BF3_BLOCK = 512

# success_rows_kernel (success.hip) has a stack: its cylinder test is a real call (obb_cylinder_overlap is __noinline__), so the link box it
# is handed by address (LR, Lc, he) and the callee's frame live in private memory, beside per-thread arrays that the non-unrolled joint
# loop indexes with a run-time joint number.  Stack arrays, not spills.  It runs once per scene, after the 255 reverse steps.  Any other
# kernel with a private segment, or this one growing, fails.  (SGPR spills go to VGPR lanes, not to memory: a kernel with SGPR spills
# and no private segment uses no scratch, so they are not checked.)
SCRATCH_ALLOWANCE = {"success_rows_kernel": 224}

_BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    path = os.path.join(LLVM, name)
    assert os.path.exists(path), f"{path} is missing (ROCm's LLVM)"
    return path


def _code_objects(fatbin: bytes):
    """the gfx950 device images of every clang offload bundle in the section (one bundle per translation unit)"""
    out, pos = [], fatbin.find(_BUNDLE_MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", fatbin, pos + len(_BUNDLE_MAGIC))
        p, end = pos + len(_BUNDLE_MAGIC) + 8, pos
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, p)
            triple = fatbin[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            end = max(end, pos + off + size)
            if triple.startswith("hip") and triple.endswith("gfx950"):
                out.append(fatbin[pos + off:pos + off + size])
        pos = fatbin.find(_BUNDLE_MAGIC, max(end, p))
    return out


def _kernel_metadata(notes: str):
    """the top-level keys of each amdhsa.kernels entry of `llvm-readelf --notes` (the nested argument lists are skipped)"""
    kernels, cur = [], None
    for line in notes.splitlines():
        if line.startswith("  - ."):  # a new kernel entry; its first key sits on the same line
            cur = {}
            kernels.append(cur)
            line = "    " + line[4:]
        elif not line.startswith("    "):
            cur = None
        m = re.match(r"^    \.([a-z_]+):\s+(\S.*)$", line) if cur is not None else None
        if m:
            v = m.group(2).strip()
            cur[m.group(1)] = int(v) if re.fullmatch(r"-?\d+", v) else v
    return [k for k in kernels if "name" in k]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: [metadata dict per occurrence]} over all gfx950 code objects of the library"""
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    d = tmp_path_factory.mktemp("code_objects")
    fb = d / "fatbin"
    subprocess.run([_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", LIB, str(d / "lib.so")], check=True)
    cos = _code_objects(fb.read_bytes())
    assert len(cos) >= _n_shards() + 2, f"{len(cos)} gfx950 code objects, expected one per translation unit"
    out = {}
    for i, co in enumerate(cos):
        f = d / f"co{i}.o"
        f.write_bytes(co)
        notes = subprocess.run([_tool("llvm-readelf"), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
        for k in _kernel_metadata(notes):
            out.setdefault(k["name"], []).append(k)
    return out


def _n_shards():
    for line in open(os.path.join(CSRC, "kernel_instances.h")):
        if line.startswith("#define EDMP_KERNEL_SHARDS"):
            return int(line.split()[2])
    raise AssertionError("EDMP_KERNEL_SHARDS not found")


def _instances(macro):
    """the X(...) lines of `#define <macro>(X)` in kernel_instances.h, as lists of argument strings (shard first)"""
    src = open(os.path.join(CSRC, "kernel_instances.h")).read()
    m = re.search(r"#define " + macro + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", src)
    assert m, macro
    return [[a.strip() for a in x.split(",")] for x in re.findall(r"X\(([^)]*)\)", m.group(1))]


ENUMS = {"WK_K5": 0, "WK_DOWN": 1, "WK_UP": 2, "WK_K5K2": 3, "WK_K5K4": 4, "LV_DOWN": 0, "LV_UP": 1, "LV_UP_FINAL": 2, "true": 1, "false": 0}


def _template_args(mangled):
    """('bf3_conv_kernel', (0, 32, 32, 32, 7, 1)) for _ZN4edmp15bf3_conv_kernelILi0ELi32ELi32ELi32ELi7ELb1EEEv..., None if not a template"""
    m = re.match(r"_ZN4edmp(\d+)", mangled)
    if not m:
        return None
    n, p = int(m.group(1)), m.end()
    name, rest = mangled[p:p + n], mangled[p + n:]
    t = re.match(r"I((?:L[ib]n?\d+E)+)E", rest)
    if not t:
        return None
    args = tuple(int(v.replace("n", "-")) for v in re.findall(r"L[ib](n?\d+)E", t.group(1)))
    return name, args


def _instances_of(kernels, name):
    out = {}
    for sym, metas in kernels.items():
        ta = _template_args(sym)
        if ta and ta[0] == name:
            out.setdefault(ta[1], []).extend((sym, m) for m in metas)
    return out


def _key(args):
    return tuple(ENUMS[a] if a in ENUMS else int(a) for a in args)


def test_fatbin_walk_finds_every_translation_unit(kernels):
    assert len(kernels) >= 90, sorted(kernels)
    assert any(n.startswith("_ZN4edmp15bf3_conv_kernel") for n in kernels)


def test_bf3_kernels_claim_their_whole_cu(kernels):
    """one bf3_conv_kernel per EDMP_BF3_INSTANCES line, max_flat_workgroup_size 512, and VGPRs (rounded up to the granule) x 2 waves per
    SIMD = the 512-entry file: no wave of any other kernel fits on the CU beside a bf16x3 workgroup"""
    lines = _instances("EDMP_BF3_INSTANCES")
    assert len(lines) == 16
    found = _instances_of(kernels, "bf3_conv_kernel")
    waves_per_simd = BF3_BLOCK // 64 // SIMDS_PER_CU
    bad = []
    for x in lines:
        key = _key(x[1:])
        occ = found.pop(key, [])
        label = f"bf3_conv_kernel<{', '.join(x[1:])}> (shard {x[0]})"
        if len(occ) != 1:
            bad.append(f"{label}: {len(occ)} kernels in the library")
            continue
        meta = occ[0][1]
        vgpr = meta["vgpr_count"]
        alloc = -(-vgpr // VGPR_GRANULE) * VGPR_GRANULE
        if meta["max_flat_workgroup_size"] != BF3_BLOCK:
            bad.append(f"{label}: max_flat_workgroup_size {meta['max_flat_workgroup_size']} != {BF3_BLOCK}")
        if alloc * waves_per_simd != VGPR_FILE:
            bad.append(f"{label}: vgpr_count {vgpr} -> {alloc} x {waves_per_simd} waves per SIMD = {alloc * waves_per_simd} of {VGPR_FILE} registers")
    assert not found, f"bf3_conv_kernel instances not listed in EDMP_BF3_INSTANCES: {sorted(found)}"
    assert not bad, "bf16x3 kernels that no longer own their CU:\n" + "\n".join(bad)


@pytest.mark.parametrize("macro,name", [("EDMP_WIDE_INSTANCES", "wide_conv_kernel"), ("EDMP_LEVEL_INSTANCES", "level_kernel"),
                                        ("EDMP_LEVEL2_INSTANCES", "level2_kernel"), ("EDMP_BF3_INSTANCES", "bf3_conv_kernel")])
def test_every_listed_instance_is_in_the_library_once(kernels, macro, name):
    """a dropped or duplicated shard line otherwise shows only as an undefined symbol at the first launch of that instance"""
    lines = _instances(macro)
    found = _instances_of(kernels, name)
    missing = [f"{name}<{', '.join(x[1:])}> (shard {x[0]}): {len(found.get(_key(x[1:]), []))} kernels" for x in lines if len(found.get(_key(x[1:]), [])) != 1]
    assert not missing, "\n".join(missing)
    assert len({_key(x[1:]) for x in lines}) == len(lines), f"{macro} lists an instance twice"
    assert len(found) == len(lines), f"{name} instances not listed in {macro}: {sorted(set(found) - {_key(x[1:]) for x in lines})}"


def test_no_kernel_uses_scratch(kernels):
    bad = []
    for sym, metas in kernels.items():
        short = _template_args(sym)[0] if _template_args(sym) else re.sub(r"^_ZN4edmp\d+", "", sym).split("E", 1)[0]
        for m in metas:
            priv = m.get("private_segment_fixed_size", 0)
            spills = m.get("vgpr_spill_count", 0)
            if spills != 0 or m.get("uses_dynamic_stack", "false") != "false" or priv != SCRATCH_ALLOWANCE.get(short, 0):
                bad.append(f"{sym}: private segment {priv} B, {spills} VGPR spills, dynamic stack {m.get('uses_dynamic_stack')}")
    assert not bad, "\n".join(bad)
    for short in SCRATCH_ALLOWANCE:  # the allowance names a kernel that exists
        assert any(short in sym for sym in kernels), short


def test_bf3_launch_size_is_the_launch_bounds_constant():
    """host side of the claim: the kernel's __launch_bounds__, its tiling and its launch all use kBf3Threads = 512"""
    src = open(os.path.join(CSRC, "bf3.hip")).read()
    m = re.search(r"constexpr int kBf3Threads = (\d+);", src)
    assert m and int(m.group(1)) == BF3_BLOCK
    assert re.search(r"__launch_bounds__\(kBf3Threads\) void bf3_conv_kernel\(", src)
    assert "static constexpr int NTH = kBf3Threads" in src
    launcher = src[src.index("int launch_bf3_t("):]
    launcher = launcher[:launcher.index("\n}\n")]
    launch = re.findall(r"hipLaunchKernelGGL\(.*", launcher)
    assert len(launch) == 1 and "dim3(kBf3Threads), bytes" in launch[0], launch
    assert "hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg, fn, kBf3Threads, bytes)" in launcher
    assert src.count('asm volatile("v_mov_b32 v255, 0" ::: "v255");') == 1


def test_cu_claim_decision():
    """edmp_cu_claim: the host-only rule edmp_unet_load applies to every bf16x3 op (refusal otherwise, naming EDMP_BF16X3=0)"""
    from edmp_amd import _capi

    claim = _capi.load().edmp_cu_claim
    assert claim(256, 512, 40960, 1) == 1
    assert claim(249, 512, 40960, 1) == 1  # allocated in granules of 8: 249 -> 256
    assert claim(248, 512, 40960, 1) == 0  # 2 x 248: 16 registers per lane left for another kernel's wave
    assert claim(128, 512, 40960, 1) == 0
    assert claim(256, 256, 40960, 1) == 0  # one wave per SIMD: half the file free
    assert claim(128, 1024, 40960, 1) == 1  # four waves per SIMD x 128
    assert claim(256, 512, 40960, 2) == 0  # the runtime places two workgroups per CU
    assert claim(256, 512, 40960, 0) == 0  # cannot launch at all
    assert claim(0, 512, 40960, 1) == 0
    assert claim(256, 512, 0, 1) == 1



def _g16_dims(aid):
    import numpy as np

    return tuple(int(d) for d in np.load(os.path.join(ROOT, "tests", "golden", "g16_unet_archs.npz"))[f"{aid}_dims"])


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["full", "default", "A2", "A4"])
def test_runtime_sees_every_bf3_op_own_its_cu(kernels, arch):
    """What the HIP runtime reports for the bf16x3 ops of a built program (edmp_unet_op_attrs; the same numbers the build's
    CU-claim check saw): one workgroup of 512 threads per CU, and the register count of the code-object metadata above"""
    from edmp_amd.temporalunet import TemporalUNet

    dims = {"full": (32, 64, 128, 256, 512, 512), "default": (32, 64, 128, 256)}.get(arch) or _g16_dims(arch)
    net = TemporalUNet(None, 7, 32, "cuda:0", dims=dims, seed=1, max_batch=8)
    ops = [a for a in net.op_attrs() if a["name"].startswith("bf3_conv_kernel<")]
    assert ops, f"{arch} {dims}: no bf16x3 op in the program"
    meta = _instances_of(kernels, "bf3_conv_kernel")
    for a in ops:
        key = _key(a["name"][len("bf3_conv_kernel<"):-1].split(", "))
        assert len(meta.get(key, [])) == 1, a
        vgpr = meta[key][0][1]["vgpr_count"]
        print(f"[{arch}] {a['name']}: {a['regs']} VGPRs (code object {vgpr}), block {a['block']}, LDS {a['lds']} B, {a['wg_per_cu']} workgroup(s) per CU")
        assert a["wg_per_cu"] == 1 and a["block"] == BF3_BLOCK, a
        assert a["regs"] == vgpr, (a, vgpr)
    assert all(a["regs"] == 0 and a["wg_per_cu"] == 0 for a in net.op_attrs() if not a["name"].startswith("bf3_conv_kernel<"))
