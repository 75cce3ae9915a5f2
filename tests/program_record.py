"""The cells of tests/golden/unet_program_parent.json and what is kept of one BOUND model (one definition for the recorder,
scripts/record_program_parent.py, and the test, tests/test_gpu_program_record.py).

A cell is an (architecture, builder-switch setting) pair of tests/plan_record.py: TINY and A1..A10 under all eighteen settings, FULL
under four.  Of the model built for it from a seeded state dict (max_batch = 4) the record keeps everything the host side of the build
decides: the SHA-256 of the packed weight image, per program op its kernel name, issued FLOPs, bf16-pipe FLOPs and reported kernel
attributes, the five FLOP totals, and for every activation tap id its (C, L) or "absent".  An architecture the builder refuses under a
setting is kept as its error message.  No forward runs: the record holds the layer program, not the kernels."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from tests import plan_record as R

RECORD = os.path.join(R.HERE, "golden", "unet_program_parent.json")
MAX_BATCH = 4
SMALL = ("TINY",) + tuple(f"A{i}" for i in range(1, 11))
FULL_SETTINGS = ("default", "BF16X3=0", "NO_FUSED", "LEVEL_MERGE=0")
SEEDS = {"TINY": 71, "FULL": 72}  # A1..A10: the seed tests/golden/g16_unet_archs.npz keeps


def cells():
    """every (architecture, setting) name pair of the record, in its order"""
    return [(a, s) for a in SMALL for s in R.SETTINGS] + [("FULL", s) for s in FULL_SETTINGS]


def seed_of(aid):
    if aid in SEEDS:
        return SEEDS[aid]
    return int(np.load(os.path.join(R.HERE, "golden", "g16_unet_archs.npz"))[f"{aid}_seed"])


def state_dict(aid):
    from edmp_amd import weights as W

    cin, td, dims, _ = R.archs()[aid]
    return W.init_state_dict(seed_of(aid), cin, td, dims)


def build(aid, setting, sd=None, device="cuda:0", model_dir=None):
    """the model of one cell, the builder switches set around its construction only (model_dir: load it from that directory instead)"""
    from edmp_amd.temporalunet import TemporalUNet

    cin, td, dims, n = R.archs()[aid]
    saved = {k: os.environ.pop(k, None) for k in R.SWITCHES}
    try:
        os.environ.update(R.SETTINGS[setting])
        net = TemporalUNet(model_dir, cin, td, device, dims=dims, state_dict=None if model_dir else (state_dict(aid) if sd is None else sd),
                           max_batch=MAX_BATCH, horizon=n)
    finally:
        for k in R.SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return net


def tap_ids(n_levels):
    return list(range(n_levels)) + [100] + [200 + j for j in range(n_levels - 1)]


def tap_shapes(net):
    """tap id -> [C, L], or "absent" where the program keeps no HBM copy (the shape query: a null output of capacity 0)"""
    from edmp_amd import _capi

    net._bind()
    out = {}
    for w in tap_ids(len(net.dims)):
        c, l = C.c_int(), C.c_int()
        try:
            _capi.check(net.ctx.lib.edmp_unet_read_activation_dev(net.ctx.h, w, MAX_BATCH, None, 0, C.byref(c), C.byref(l)), "edmp_unet_read_activation_dev")
            out[str(w)] = [c.value, l.value]
        except _capi.EdmpError:
            out[str(w)] = "absent"
    return out


def image(net):
    """(layout id, the packed weight image as edmp_unet_read_packed returns it)"""
    from edmp_amd import _capi

    net._bind()
    layout = C.c_int()
    n = net.ctx.lib.edmp_unet_packed_size(net.ctx.h, C.byref(layout))
    blob = np.empty(n, dtype=np.float32)
    _capi.check(net.ctx.lib.edmp_unet_read_packed(net.ctx.h, _capi.as_pf(blob), n), "edmp_unet_read_packed")
    return layout.value, blob


def describe(net):
    """what the record keeps of a bound model (plain JSON types; floats are Python floats: exact doubles through json)"""
    layout, blob = image(net)
    ops = net.ctx.prof_ops()
    bf16 = net.ctx.prof_ops_bf16()
    attrs = net.op_attrs()
    assert len(ops) == len(bf16) == len(attrs)
    nominal, issued = net.flops_per_trajectory()
    f32, b16 = net.flops_by_pipe()
    return {
        "layout": layout,
        "n_packed": int(blob.size),
        "image_sha256": hashlib.sha256(blob.tobytes()).hexdigest(),
        "ops": [[n, fl, fb] for (n, _, _, fl), fb in zip(ops, bf16)],
        "attrs": [[a["name"], a["regs"], a["block"], a["lds"], a["wg_per_cu"]] for a in attrs],
        "flops": {"nominal": nominal, "issued": issued, "direct": net.flops_direct_form(), "f32_pipe": f32, "bf16_pipe": b16},
        "taps": tap_shapes(net),
    }


def cell(aid, setting, sd=None, device="cuda:0"):
    """the record's entry of one cell: describe() of its model, or the builder's refusal"""
    from edmp_amd import _capi

    try:
        net = build(aid, setting, sd=sd, device=device)
    except _capi.EdmpError as e:
        return {"refused": str(e)}
    return describe(net)


def pack(by_cell):
    """{"ARCH/setting": entry} -> the file's body, every value kept once.  Many cells are the same model (a switch that governs no
    layer of the architecture) and a program repeats few distinct ops: "rows" holds each distinct [ops row, attrs row] pair, an
    entry's "program" lists its ops as indices into it, "entries" holds each distinct entry and "cells" the index of each cell's."""
    rows, entries, cells = {}, {}, {}
    for name, e in by_cell.items():
        if "refused" not in e:
            e = {k: v for k, v in e.items() if k not in ("ops", "attrs")} | {
                "program": [rows.setdefault(json.dumps(r), len(rows)) for r in zip(e["ops"], e["attrs"])]}
        cells[name] = entries.setdefault(json.dumps(e, sort_keys=True), len(entries))
    return {"rows": [json.loads(k) for k in rows], "entries": [json.loads(k) for k in entries], "cells": cells}


def unpack(record):
    """the file -> {"ARCH/setting": entry}, each entry as describe() or cell() gave it (through json)"""
    def entry(e):
        if "refused" in e:
            return e
        pairs = [record["rows"][i] for i in e["program"]]
        return {k: v for k, v in e.items() if k != "program"} | {"ops": [p[0] for p in pairs], "attrs": [p[1] for p in pairs]}

    return {name: entry(record["entries"][i]) for name, i in record["cells"].items()}
