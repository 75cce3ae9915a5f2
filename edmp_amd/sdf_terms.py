"""The optional terms of the sphere signed-distance guide (csrc/sdf.hip), each stated once: plain data that guide_cfg (YAML -> per-row
arrays), guide (row arrays -> host tables -> the library's setters) and dist (row shards) read.

TERMS is in launch order (sdf_overlay) = setter order (_SlotObject._set_sdf).  ``extra`` names what a term's setter takes beside its row
arrays and guide.sdf_tables returns with them (the self term's pair mask).  A term's first key is its weight: the term's keys enter
``guide_cfgs`` only when some guide sets it > 0, and a weight > 0 is allowed only on an SDF row.  Per key:
  hyper      name under ``hyperparameters.sdf`` and in the dict guide.sdf_tables returns
  cfg        key in ``guide_cfgs``
  cfg_dtype  dtype there (sdf_goal_window is int64: the committed digests pin it)
  dtype      dtype in the host tables, as the setter takes it
  default    value of a guide that does not name the key
  pair       False: one scalar per row; True: [m0, m1], spread by linspace over the T steps
  check      "nonneg": finite and >= 0; "real": the same and a real number by type (a bool or a string is refused before its value is
             looked at); "int": an integer in lo..hi (hi None: no upper end); "int_weighted": the same, but the row arrays are held to it
             only where the row's weight is > 0 (a guide's YAML always is)
"""
from collections import namedtuple

import numpy as np

from ._capi import MAX_SWEEP_SUBSTEPS

Key = namedtuple("Key", "hyper cfg cfg_dtype dtype default pair check lo hi", defaults=(None, None))
Term = namedtuple("Term", "name setter keys extra", defaults=((),))

TERMS = (
    Term("self", "edmp_sdf_set_self", (
        Key("self_weight", "sdf_self_weight", np.float64, np.float64, 0.0, False, "nonneg"),
        Key("self_margin", "sdf_self_margin", np.float64, np.float64, (0.0, 0.0), True, "nonneg")), extra=("self_mask",)),
    Term("goal", "edmp_sdf_set_goal", (
        Key("goal_weight", "sdf_goal_weight", np.float64, np.float64, 0.0, False, "nonneg"),
        Key("goal_rotation", "sdf_goal_rotation", np.float64, np.float64, 0.0, False, "nonneg"),
        Key("goal_window", "sdf_goal_window", np.int64, np.int32, 8, False, "int", 1))),
    Term("sweep", "edmp_sdf_set_sweep", (
        Key("sweep_weight", "sdf_sweep_weight", np.float64, np.float64, 0.0, False, "real"),
        Key("sweep_substeps", "sdf_sweep_substeps", np.int32, np.int32, 4, False, "int_weighted", 2, MAX_SWEEP_SUBSTEPS))),
)
TERM = {t.name: t for t in TERMS}
BASE_CFG_KEYS = ("sdf_rows", "sdf_margin", "smoothness")  # present whenever some guide uses the method
CFG_KEYS = tuple(k.cfg for t in TERMS for k in t.keys)


def is_int(k: Key) -> bool:
    return k.check in ("int", "int_weighted")


def span(k: Key) -> str:
    """the allowed values of an integer key as a message names them"""
    return f"an integer >= {k.lo}" if k.hi is None else f"an integer in {k.lo}..{k.hi}"


def default_rows(k: Key, n: int, T: int):
    """n rows of a key that nobody brings, in the host tables' dtype"""
    return np.tile(np.linspace(*k.default, T), (n, 1)) if k.pair else np.full(n, k.default, dtype=k.dtype)
