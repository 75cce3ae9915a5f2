"""The activation taps of TemporalUNet.activation and the rule for a tap a layer program keeps no HBM copy of.  Shared by
tests/test_gpu_archs.py and tests/test_gpu_hostile_activations.py.  A plain module: no fixtures, no pytest hooks."""


def tap_ids(n_levels):
    """every tap of a network of n_levels: the down levels, the middle block (100), the up levels (200 + j)"""
    return list(range(n_levels)) + [100] + [200 + j for j in range(n_levels - 1)]


def tap_key(which):
    """the oracle's trace key of a tap id"""
    return "mid" if which == 100 else f"down{which}" if which < 100 else f"up{which - 200}"


def missing_tap_explained(which, n_levels, names):
    """a tap the program has no HBM copy of: level 0's output handed to level 1 in LDS (level2_kernel bit 0), the up level merged
    into the last one (bit 1), and the last up level itself (its output feeds final_conv.0 inside the same launch)"""
    if which == 0:
        return any(s.startswith("level2_kernel<0") for s in names)
    if which == 200 + n_levels - 3:
        return any(s.startswith("level2_kernel<1") for s in names)
    if which == 200 + n_levels - 2:
        return any(s.startswith("level_kernel<2") or s.startswith("level2_kernel<1") for s in names)
    return False
