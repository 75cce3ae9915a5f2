"""The (architecture, builder-switch setting) grid of tests/golden/unet_plan_record.json and the host-only call that describes one
cell (edmp_unet_plan_describe).  Shared by tests/test_plan_record.py and scripts/gen_plan_record.py."""
import hashlib
import os

import numpy as np

from tests.util import FULL_DIMS, T, TINY_DIMS

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "golden", "unet_plan_record.json")
SWITCHES = ("EDMP_BF16X3", "EDMP_MS16", "EDMP_LEVEL_MERGE", "EDMP_LEVEL_SB", "EDMP_NO_KARATSUBA", "EDMP_NO_FUSED", "EDMP_NO_RESFOLD", "EDMP_NO_LEVEL")

SETTINGS = {"default": {}}
SETTINGS.update({f"BF16X3={m}": {"EDMP_BF16X3": m} for m in ("0", "0x7", "0x3f", "0x7f", "0xbf")})
SETTINGS.update({f"BF16X3=0,MS16={m}": {"EDMP_BF16X3": "0", "EDMP_MS16": m} for m in ("0", "0x1f")})
SETTINGS["NO_KARATSUBA"] = {"EDMP_NO_KARATSUBA": "1"}
SETTINGS["NO_KARATSUBA,BF16X3=0"] = {"EDMP_NO_KARATSUBA": "1", "EDMP_BF16X3": "0"}
SETTINGS.update({f"NO_{k}": {f"EDMP_NO_{k}": "1"} for k in ("RESFOLD", "LEVEL", "FUSED")})
SETTINGS.update({f"LEVEL_MERGE={m}": {"EDMP_LEVEL_MERGE": m} for m in ("0", "1", "2")})
SETTINGS.update({f"LEVEL_SB={d}": {"EDMP_LEVEL_SB": d} for d in ("2222", "4444")})


def archs():
    """name -> (input_dim, time_dim, dims, horizon): TINY, FULL and G16's A1..A10"""
    g = np.load(os.path.join(HERE, "golden", "g16_unet_archs.npz"))
    out = {"TINY": (7, 32, TINY_DIMS, 50), "FULL": (7, 32, FULL_DIMS, 50)}
    for a in (f"A{i}" for i in range(1, 11)):
        out[a] = (int(g[f"{a}_input_dim"]), int(g[f"{a}_time_dim"]), tuple(int(d) for d in g[f"{a}_dims"]), int(g[f"{a}_horizon"]))
    return out


def describe(arch, setting):
    """what the record keeps of one cell: layout id, image floats, count per kernel name, SHA-256 of the ordered name list"""
    from edmp_amd import _capi

    cin, td, dims, n = arch
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        os.environ.update(setting)
        names, layout, size = _capi.plan_describe(cin, td, dims, n, T)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    counts = {k: names.count(k) for k in sorted(set(names))}
    return {"layout": layout, "n_packed": size, "counts": counts, "sha256": hashlib.sha256("\n".join(names).encode()).hexdigest()}
