"""ctypes binding of libedmp_hip.so (include/edmp_hip.h).  Fails loudly when the library is missing or does not
load — there is no CPU fallback for the product path."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libedmp_hip.so")

MAX_LEVELS = 8
MAX_SCENES = 16  # EDMP_MAX_SCENES
MAX_OBSTACLES = 64  # EDMP_MAX_OBSTACLES
MAX_SPHERES = 128  # EDMP_MAX_SPHERES
MAX_SWEEP_SUBSTEPS = 64  # EDMP_MAX_SWEEP_SUBSTEPS
MAX_REPAIR_ITERS = 1024  # EDMP_MAX_REPAIR_ITERS
MAX_TIMED_SAMPLES = 1048576  # EDMP_MAX_TIMED_SAMPLES


class UNetDesc(C.Structure):
    _fields_ = [
        ("input_dim", C.c_int32),
        ("time_dim", C.c_int32),
        ("n_levels", C.c_int32),
        ("dims", C.c_int32 * MAX_LEVELS),
        ("horizon", C.c_int32),
        ("T", C.c_int32),
    ]


class EdmpError(RuntimeError):
    rc = None  # status code of the failing C-ABI call (include/edmp_hip.h), None for errors raised on the Python side


class EdmpLayoutError(EdmpError):
    """EDMP_ERR_LAYOUT: a packed weight image written by another library version or under other builder switches"""


ERR_LAYOUT = -4


_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_pd, _pf, _pi32 = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
_pu64 = C.POINTER(C.c_uint64)

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)  # edmp_allreduce_fn(user, hip_stream, sumsq_dev)

# name -> (restype, argtypes); every symbol include/edmp_hip.h declares
SIGNATURES = {
    "edmp_last_error": (C.c_char_p, []),
    "edmp_version": (_i, []),
    "edmp_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "edmp_ctx_destroy": (None, [_vp]),
    "edmp_ctx_set_stream": (_i, [_vp, _vp]),
    "edmp_ctx_synchronize": (_i, [_vp]),
    "edmp_unet_param_count": (C.c_int64, [C.POINTER(UNetDesc)]),
    "edmp_unet_load": (_i, [_vp, C.POINTER(UNetDesc), _pf, C.c_int64, _i]),
    "edmp_unet_forward_dev": (_i, [_vp, _vp, _i, _i, _vp]),
    "edmp_unet_read_activation_dev": (_i, [_vp, _i, _i, _vp, C.c_int64, C.POINTER(_i), C.POINTER(_i)]),
    "edmp_unet_flops": (_i, [_vp, _pd, _pd]),
    "edmp_scene_set": (_i, [_vp, _pd, _i, _pd, _pd, _i, _i, _pf, _pf, _pf]),
    "edmp_rows_set": (_i, [_vp, _pi32, _pf, _pd, _pd, _i, _i]),
    "edmp_scene_read_aabbs": (_i, [_vp, _i, _i, _pf]),
    "edmp_guide_cost_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "edmp_guide_swept_cost_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _pf, _pf, _vp]),
    "edmp_guide_gradient_dev": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _vp, _vp]),
    "edmp_row_swept_volumes_dev": (_i, [_vp, _vp, _i, _i, _pd, _pd, _vp, C.POINTER(_i)]),
    "edmp_scene_set_shapes": (_i, [_vp, _pi32, _i]),
    "edmp_success_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _pd, _vp, _vp, _vp, _pi32]),
    "edmp_self_collision_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _pd, _pi32, _vp, _vp]),
    "edmp_metrics_rows_dev": (_i, [_vp, _vp, _i, _i, _d, _pd, _vp]),
    "edmp_select_row_dev": (_i, [_vp, _vp, _vp, _i, _d, C.POINTER(_i)]),
    "edmp_sampler_init": (_i, [_vp, _i, _d]),
    "edmp_sampler_read_schedule": (_i, [_vp, _pd, _pd, _pd]),
    "edmp_sampler_set_condition": (_i, [_vp, _i]),
    "edmp_psample_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "edmp_step_a_dev": (_i, [_vp, _vp, _vp, _i, _i, _pd, _pd, _i, _vp, _vp]),
    "edmp_step_b_dev": (_i, [_vp, _vp, _i, _i, _pd, _pd, _vp]),
    "edmp_sumsq_ptr_dev": (_vp, [_vp]),
    "edmp_denoise_guided_dev": (_i, [_vp, _vp, _i, _pd, _pd, _i, _i, _i, _vp]),
    "edmp_denoise_guided_segment_dev": (_i, [_vp, _vp, _i, _pd, _pd, _i, _i, _i, _i, _i, _vp]),
    "edmp_denoise_guided_rng_dev": (_i, [_vp, C.c_uint64, _i, _pd, _pd, _i, _i, _i, _vp]),
    "edmp_rng_normal_dev": (_i, [_vp, C.c_uint64, _i, _i, _i, _i, _vp]),
    "edmp_denoise_guided_rng_segment_dev": (_i, [_vp, C.c_uint64, _i, _pd, _pd, _i, _i, _i, _i, _i, _vp]),
    "edmp_denoise_scenes_rng_dev": (_i, [_vp, _pu64, _i, _i, _pd, _pd, _i, _i, _i, _vp]),
    "edmp_denoise_scenes_rng_segment_dev": (_i, [_vp, _pu64, _i, _i, _pd, _pd, _i, _i, _i, _i, _i, _vp]),
    "edmp_sampler_seed_rng_dev": (_i, [_vp, _vp, _i, C.c_uint64, _i, _i, _pd, _pd, _i, _i, _vp]),
    "edmp_sampler_seed_scenes_rng_dev": (_i, [_vp, _vp, _i, _pu64, _i, _i, _i, _pd, _pd, _i, _i, _vp]),
    "edmp_sampler_set_graph": (_i, [_vp, _i]),
    "edmp_scene_batch_set": (_i, [_vp, _i, _pi32, _pd, _pi32, _pd, _pd, _i, _pf, _pf, _pf]),
    "edmp_denoise_scenes_dev": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _i, _vp]),
    "edmp_denoise_scenes_segment_dev": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _i, _i, _i, _vp]),
    "edmp_sampler_seed_dev": (_i, [_vp, _vp, _i, _vp, _i, _pd, _pd, _i, _i, _vp]),
    "edmp_sampler_seed_scenes_dev": (_i, [_vp, _vp, _i, _vp, _i, _i, _pd, _pd, _i, _i, _vp]),
    "edmp_scene_batch_set_shapes": (_i, [_vp, _pi32, _i]),
    "edmp_scenes_swept_volumes_dev": (_i, [_vp, _vp, _i, _i, _i, _pd, _pd, _vp, C.POINTER(_i)]),
    "edmp_scenes_select_rows_dev": (_i, [_vp, _vp, _vp, _i, _i, _d, C.POINTER(_i)]),
    "edmp_scenes_success_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _pd, _vp, _vp, _vp, _pi32]),
    "edmp_scenes_goal_filter_dev": (_i, [_vp, _vp, _i, _pi32, _pd, _d, _vp, _vp, C.POINTER(_i)]),
    "edmp_ik_solve_dev": (_i, [_vp, _pd, _i, _pi32, _vp, _pd, _i, _d, _d, _d, _d, _vp, _vp, _vp]),
    "edmp_ik_compact_dev": (_i, [_vp, _vp, _vp, _i, _pi32, _vp, _pi32]),
    "edmp_q_sample_dev": (_i, [_vp, _vp, _vp, _pi32, _i, _i, _i, _i, _i, _vp, _vp]),
    "edmp_unet_packed_size": (C.c_int64, [_vp, C.POINTER(C.c_int)]),
    "edmp_unet_read_packed": (_i, [_vp, _pf, C.c_int64]),
    "edmp_unet_load_packed": (_i, [_vp, C.POINTER(UNetDesc), _pf, C.c_int64, _i, _i]),
    "edmp_unet_plan_describe": (_i, [C.POINTER(UNetDesc), _i, C.POINTER(C.c_int), C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "edmp_unet_flops_direct": (_i, [_vp, _pd]),
    "edmp_unet_flops_pipes": (_i, [_vp, _pd, _pd]),
    "edmp_prof_ops_bf16": (_i, [_vp, _i, C.POINTER(C.c_int), _pd]),
    "edmp_unet_slot": (_i, [_vp, C.c_uint64]),
    "edmp_guide_slot": (_i, [_vp, C.c_uint64]),
    "edmp_argmin_dev": (_i, [_vp, _vp, _i, C.POINTER(C.c_int)]),
    "edmp_sdf_set": (_i, [_vp, _pf, _i, _pi32, _pd, _pd, _i, _i]),
    "edmp_sdf_set_self": (_i, [_vp, _pi32, _pd, _pd, _i, _i]),
    "edmp_sdf_self_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "edmp_sdf_set_goal": (_i, [_vp, _pd, _pd, _pi32, _pd, _pd, _i]),
    "edmp_sdf_goal_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "edmp_sdf_set_sweep": (_i, [_vp, _pd, _pi32, _i]),
    "edmp_sdf_sweep_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _pd, _pd, _i, _vp, _vp]),
    "edmp_scenes_sdf_sweep_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _pd, _pd, _i, _vp, _vp]),
    "edmp_sdf_repair_rows_dev": (_i, [_vp, _vp, _i, _i, _pd, _pd, _pi32, _i, _i, _i, _d, _d, _d, _d, _vp, _vp, _vp]),
    "edmp_scenes_sdf_repair_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _pd, _pd, _pi32, _i, _i, _i, _d, _d, _d, _d, _vp, _vp, _vp]),
    "edmp_shortcut_rows_dev": (_i, [_vp, _vp, _i, _i, _pi32, _i, _i, _i, _d, _pd, _vp, _vp, _vp, _vp, _i]),
    "edmp_scenes_shortcut_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _pi32, _i, _i, _i, _d, _pd, _vp, _vp, _vp, _vp, _i]),
    "edmp_shortcut_rows_self_dev": (_i, [_vp, _vp, _i, _i, _pi32, _i, _i, _i, _d, _pd, _vp, _vp, _vp, _vp, _i, _pi32, _vp]),
    "edmp_scenes_shortcut_rows_self_dev": (_i, [_vp, _vp, _i, _i, _i, _pi32, _i, _i, _i, _d, _pd, _vp, _vp, _vp, _vp, _i, _pi32, _vp]),
    "edmp_certify_rows_dev": (_i, [_vp, _vp, _i, _i, _pi32, _i, _i, _d, _pd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pd]),
    "edmp_scenes_certify_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _pi32, _i, _i, _d, _pd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pd]),
    "edmp_time_rows_dev": (_i, [_vp, _vp, _i, _i, _pd, _pd, _pd, _vp, _vp, _vp, _vp, _vp, _vp]),
    "edmp_sample_rows_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _pi32, _i, _d, _i, _vp, _vp, _vp]),
    "edmp_blend_rows_dev": (_i, [_vp, _vp, _i, _i, _pi32, _i, _pd, _pd, _pd, _pd, _d, _i, _i, _pd, _vp, _vp, _vp, _vp]),
    "edmp_scenes_blend_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _pi32, _i, _pd, _pd, _pd, _pd, _d, _i, _i, _pd, _vp, _vp, _vp, _vp]),
    "edmp_blend_rows_self_dev": (_i, [_vp, _vp, _i, _i, _pi32, _i, _pd, _pd, _pd, _pd, _d, _i, _i, _pd, _vp, _vp, _vp, _vp, _pi32, _vp]),
    "edmp_scenes_blend_rows_self_dev": (_i, [_vp, _vp, _i, _i, _i, _pi32, _i, _pd, _pd, _pd, _pd, _d, _i, _i, _pd, _vp, _vp, _vp, _vp, _pi32, _vp]),
    "edmp_time_blended_rows_dev": (_i, [_vp, _vp, _i, _i, _vp, _pd, _pd, _pd, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "edmp_sample_blended_rows_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _pi32, _i, _d, _i, _vp, _vp, _vp]),
    "edmp_sdf_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _pd, _pd, _vp, _vp]),
    "edmp_scene_batch_set_sdf": (_i, [_vp, _pf, _i, _pi32, _pd, _pd, _i, _i, _i]),
    "edmp_scenes_sdf_rows_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _pd, _pd, _vp, _vp]),
    "edmp_sampler_set_allreduce": (_i, [_vp, _vp, _vp]),
    "edmp_rccl_load": (_i, [C.c_char_p]),
    "edmp_rccl_unique_id": (_i, [_vp]),
    "edmp_rccl_attach": (_i, [_vp, _vp, _i, _i]),
    "edmp_rccl_attach_comm": (_i, [_vp, _vp]),
    "edmp_rccl_enable": (_i, [_vp, _i]),
    "edmp_rccl_detach": (_i, [_vp]),
    "edmp_rccl_info": (_i, [_vp, _pi32]),
    "edmp_sampler_allreduce_stats": (_i, [_vp, C.POINTER(C.c_uint64), _i]),
    "edmp_prof_enable": (_i, [_vp, _i]),
    "edmp_prof_read": (_i, [_vp, _pd, C.POINTER(C.c_int64), _i]),
    "edmp_prof_ops": (_i, [_vp, _i, C.POINTER(C.c_int), _pd, C.POINTER(C.c_int64), _pd, C.c_char_p]),
    "edmp_unet_op_attrs": (_i, [_vp, _i, C.POINTER(C.c_int), C.c_char_p, _pi32, _pi32, _pi32, _pi32]),
    "edmp_cu_claim": (_i, [_i, _i, _i, _i]),
}

_lib = None


def load():
    """dlopen libedmp_hip.so (built by __graft_entry__.build()).  Raises EdmpError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EdmpError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  edmp_amd has no CPU fallback."
        )
    # PyTorch-ROCm carries its own libamdhip64: map it FIRST, so that the process has ONE HIP runtime (our library then binds to the copy
    # already loaded).  In the other order - this library pulling /opt/rocm's runtime, torch its own afterwards (what
    # `python __graft_entry__.py smoke` did: build() loads the library before anything imported torch) - the process holds two runtimes
    # and the second one reports "no ROCm-capable device".  A host without torch (tests/c_abi) links the system runtime alone.
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover
        pass
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise EdmpError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise EdmpError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().edmp_last_error()
        err = (EdmpLayoutError if rc == ERR_LAYOUT else EdmpError)(f"{what or 'libedmp_hip'} failed (rc={rc}): {msg.decode() if msg else '?'}")
        err.rc = rc
        raise err


def as_pd(a):
    return a.ctypes.data_as(_pd)


def as_pf(a):
    return a.ctypes.data_as(_pf)


def as_pi32(a):
    return a.ctypes.data_as(_pi32)


def plan_describe(input_dim, time_dim, dims, horizon, T):
    """(kernel names per op, layout id, packed-image floats) of the layer program edmp_unet_load would build for this architecture
    under the current builder switches (edmp_unet_plan_describe: host-only, needs no GPU)."""
    lib = load()
    d = UNetDesc()
    d.input_dim, d.time_dim, d.n_levels, d.horizon, d.T = input_dim, time_dim, len(dims), horizon, T
    for i, v in enumerate(dims):
        d.dims[i] = v
    n, layout, size = C.c_int(), C.c_int(), C.c_int64()
    check(lib.edmp_unet_plan_describe(C.byref(d), 0, C.byref(n), None, None, None), "edmp_unet_plan_describe")
    names = C.create_string_buffer(max(n.value, 1) * 64)
    check(lib.edmp_unet_plan_describe(C.byref(d), n.value, C.byref(n), names, C.byref(layout), C.byref(size)), "edmp_unet_plan_describe")
    return [names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode() for i in range(n.value)], layout.value, size.value
