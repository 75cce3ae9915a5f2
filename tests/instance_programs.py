"""The kernel instances csrc/kernel_instances.h lists, and the table of programs (architecture, builder switches) that between them
launch every one of them.  Shared by tests/test_instance_coverage_host.py (CPU: the table reaches every listed instance) and
tests/test_gpu_instances.py (GPU: every program of the table against the oracle).  A plain module: no fixtures, no pytest hooks.

The rule: an instance listed in kernel_instances.h has a row of PROGRAMS whose plan launches it.  Adding an instance without a
program that runs it fails tests/test_instance_coverage_host.py on the CPU; the row then gets its GPU checks from the parametrised
tests of tests/test_gpu_instances.py."""
import collections
import fnmatch
import os
import re

from tests import plan_record as R

CSRC = os.path.join(os.path.dirname(R.HERE), "edmp_amd", "csrc")

# One row per program.  arch: "FULL" or an id of tests/golden/g16_unet_archs.npz - the small architectures where they reach the
# instance (the float64 oracle of A2 / A3 is cheap), FULL for what only six levels reach.  env: the builder switches.  swept_by: the
# test that already holds the program's forward to the oracle at ragged batches (for those rows tests/test_gpu_instances.py only checks
# that the bound program launches what the row is there for; every other row gets the sweep).  there_for: the listed instances this
# row answers for, as fnmatch patterns over their names - every listed instance belongs to exactly one row, whose plan launches it.
Program = collections.namedtuple("Program", "arch env swept_by there_for why")
PROGRAMS = (
    Program("A2", {"EDMP_LEVEL_MERGE": "0", "EDMP_LEVEL_SB": "4444"}, None,
            ("level_kernel<0, 32, 50, 4, 8>", "level_kernel<0, 64, 25, 4, 32>", "level_kernel<1, 64, 13, 4, 256>"),
            "the four-sample level kernels, one launch per level"),
    Program("A3", {"EDMP_LEVEL_MERGE": "0", "EDMP_LEVEL_SB": "4444"}, None, ("level_kernel<2, 32, 25, 4, 128>",),
            "the four-sample LV_UP_FINAL kernel (the fused step tail) in a net of a few launches"),
    Program("A2", {"EDMP_LEVEL_MERGE": "0", "EDMP_LEVEL_SB": "2222"}, None,
            ("level_kernel<0, 32, 50, 2, 8>", "level_kernel<0, 64, 25, 2, 32>", "level_kernel<1, 64, 13, 2, 256>", "level_kernel<2, 32, 25, 2, 128>"),
            "the two-sample level kernels, one launch per level"),
    Program("A2", {"EDMP_NO_KARATSUBA": "1", "EDMP_BF16X3": "0"}, None, ("wide_conv_kernel<0, 32, *, 4, *>",),
            "the direct-form fp32 Conv1dBlocks at L = 4"),
    Program("FULL", {}, "tests/test_gpu_parity.py::test_full_unet_fused_kernels_vs_oracle_ragged",
            ("bf3_conv_kernel<*", "level2_kernel<*", "wide_conv_kernel<3, *"),
            "the default program of the flagship net: every bf16x3 instance, both merged pairs, the L = 2 Karatsuba form"),
    Program("FULL", {"EDMP_NO_KARATSUBA": "1"}, "tests/test_gpu_parity.py::test_karatsuba_forms_with_adversarial_weights",
            ("wide_conv_kernel<0, 32, 64, 64, 2, *>",), "the direct form at L = 2"),
    Program("FULL", {"EDMP_BF16X3": "0", "EDMP_MS16": "0"}, "tests/test_gpu_parity.py::test_sixteen_sample_tiles_of_the_direct_form_instances",
            ("wide_conv_kernel<4, *", "wide_conv_kernel<0, 16, 32, 16, *", "wide_conv_kernel<0, 32, 32, 32, 7, *>", "wide_conv_kernel<1, 32, *",
             "wide_conv_kernel<2, 32, *", "wide_conv_kernel<1, 16, 32, 16, 13, false>", "wide_conv_kernel<2, 16, 32, 16, 7, false>"),
            "the fp32 position-tile kernels: 32-sample tiles at 256 / 512 channels, the 128-channel levels, the nested Karatsuba form at L = 4"),
    Program("FULL", {"EDMP_BF16X3": "0", "EDMP_MS16": "0x1f"}, "tests/test_gpu_parity.py::test_sixteen_sample_tiles_of_the_direct_form_instances",
            ("wide_conv_kernel<0, 16, 32, 32, 7, *>", "wide_conv_kernel<1, 16, 32, 32, 7, false>", "wide_conv_kernel<2, 16, 32, 32, 4, false>",
             "wide_conv_kernel<1, 16, 64, 64, 4, false>", "wide_conv_kernel<2, 16, 64, 64, 2, false>"),
            "16-sample tiles of the fp32 direct-form instances at 256 / 512 channels"),
)


def program_id(row):
    """(also of a plain (arch, env) pair)"""
    return row[0] + "/" + (",".join(f"{k[5:]}={v}" for k, v in row[1].items()) or "default")


def there_for(row, listed=None):
    """the listed instances a row answers for (its patterns expanded over kernel_instances.h)"""
    listed = listed_instances() if listed is None else listed
    return [n for n in listed if any(fnmatch.fnmatchcase(n, pat) for pat in row.there_for)]


def _enum(path, name):
    """name -> value of `enum <name> { A = 0, B = 1, ... };` in a source file, read as text"""
    text = open(os.path.join(CSRC, path)).read()
    m = re.search(r"enum\s+" + name + r"\s*(?::\s*\w+\s*)?\{([^}]*)\}", text)
    assert m, (path, name)
    out = {}
    for item in m.group(1).split(","):
        k, v = item.split("=")
        out[k.strip()] = int(v.strip(), 0)
    return out


def _xmacro_rows(text, macro):
    """the argument tuples of the X(...) rows of `#define <macro>(X) ...` (a backslash-continued block)"""
    m = re.search(r"#define\s+" + macro + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", text)
    assert m, macro
    rows = [tuple(a.strip() for a in r.split(",")) for r in re.findall(r"\bX\(([^)]*)\)", m.group(1))]
    assert rows, macro
    return rows


def listed_instances():
    """every instance of kernel_instances.h, named as prof_ops() / edmp_unet_plan_describe print it (csrc/unet.hip: op_kernel_name)"""
    text = open(os.path.join(CSRC, "kernel_instances.h")).read()
    kinds, modes = _enum("wide.hip", "WideKind"), _enum("params.h", "LevelMode")
    names = []
    for macro, family in (("EDMP_WIDE_INSTANCES", "wide"), ("EDMP_BF3_INSTANCES", "bf3")):
        for row in _xmacro_rows(text, macro):
            _, kind, ms, cg, gs, lin, res = row
            assert res in ("true", "false"), row
            names.append(f"{family}_conv_kernel<{kinds[kind]}, {int(ms)}, {int(cg)}, {int(gs)}, {int(lin)}, {res}>")
    for row in _xmacro_rows(text, "EDMP_LEVEL_INSTANCES"):
        _, mode, c, l, sb, cin = row
        names.append(f"level_kernel<{modes[mode]}, {int(c)}, {int(l)}, {int(sb)}, {int(cin)}>")
    for row in _xmacro_rows(text, "EDMP_LEVEL2_INSTANCES"):
        _, ma, ca, la, cina, mb, cb, lb, cinb, sb = row
        names.append(f"level2_kernel<{modes[ma]}, {int(ca)}, {int(la)}, {int(cina)}, {modes[mb]}, {int(cb)}, {int(lb)}, {int(cinb)}, {int(sb)}>")
    return names


def launched(names):
    """the kernels a described program really launches: a merged pair is ONE launch, named at its first level; the op behind it keeps
    the name of the level_kernel instance that would run it alone (csrc/unet.hip: op_kernel_name) and is not a launch of its own"""
    out, second_of_pair = [], False
    for n in names:
        if not second_of_pair:
            out.append(n)
        else:
            assert n.startswith("level_kernel<"), n
        second_of_pair = n.startswith("level2_kernel<")
    return out


def described(row):
    """the launched kernel names of one row of PROGRAMS (or any (arch, env) pair), from the host-only plan description (no GPU)"""
    from edmp_amd import _capi
    from tests.util import T

    aid, env = row[:2]
    cin, td, dims, n = R.archs()[aid]
    saved = {k: os.environ.pop(k, None) for k in R.SWITCHES}
    try:
        os.environ.update(env)
        names, _, _ = _capi.plan_describe(cin, td, dims, n, T)
    finally:
        for k in R.SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return launched(names)
