"""ctypes binding of libcugs_hip.so (the C ABI declared in include/cugs_hip.h).

The HIP library is the product.  There is no CPU or PyTorch fallback: if the shared
object is missing or does not export a declared symbol, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CUGS_HIP_LIBRARY: full path of another build of the same C ABI (the development build libcugs_hip_dev.so, a
# maintainer's own build).  Still a HIP library or nothing.
LIB_PATH = os.environ.get("CUGS_HIP_LIBRARY") or os.path.join(_HERE, "libcugs_hip.so")

PACKED_STRIDE = 12   # CUGS_PACKED_STRIDE
GRAD_STRIDE = 16     # CUGS_GRAD_STRIDE
TILE = 16            # CUGS_TILE


class Camera(C.Structure):
    """struct cugs_camera."""
    _fields_ = [("view", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("width", C.c_int32), ("height", C.c_int32),
                ("cam_center", C.c_float * 3), ("reserved", C.c_float)]


class AdamGroup(C.Structure):
    """struct cugs_adam_group."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p),
                ("n", C.c_int64), ("lr", C.c_float), ("reserved", C.c_float)]


class AdamFused(C.Structure):
    """struct cugs_adam_fused."""
    _fields_ = [("m", C.c_void_p * 5), ("v", C.c_void_p * 5), ("lr", C.c_float * 5), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("bc1", C.c_float), ("bc2", C.c_float)]


class DensifyArray(C.Structure):
    """struct cugs_densify_array."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_floats", C.c_int32), ("mode", C.c_int32)]


DENSIFY_COPY, DENSIFY_POSITIONS, DENSIFY_SCALES, DENSIFY_STATE = 0, 1, 2, 3


class McmcFused(C.Structure):
    """struct cugs_mcmc_fused."""
    _fields_ = [("lambda_opacity", C.c_float), ("lambda_scale", C.c_float), ("noise_lr", C.c_float),
                ("gate_k", C.c_float), ("gate_t", C.c_float), ("step", C.c_uint32), ("seed", C.c_uint64),
                ("noise", C.c_void_p)]


KNN_AUTO, KNN_EXHAUSTIVE, KNN_TREE = 0, 1, 2                            # CUGS_KNN_*
MCMC_STREAM_NOISE, MCMC_STREAM_JITTER, MCMC_STREAM_SAMPLE = 0, 1, 2     # CUGS_MCMC_STREAM_*


class PoseGrad(C.Structure):
    """struct cugs_pose_grad."""
    _fields_ = [("dL_dview", C.c_void_p), ("rows", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


class ProjectionOpts(C.Structure):
    """struct cugs_projection_opts (C.pointer(block) for mcmc and pose: the field keeps the block alive)."""
    _fields_ = [("mcmc", C.POINTER(McmcFused)), ("pose", C.POINTER(PoseGrad)), ("sparse", C.c_int)]


class BlendForwardOpts(C.Structure):
    """struct cugs_blend_forward_opts."""
    _fields_ = [("zero_buf", C.c_void_p), ("zero_bytes", C.c_size_t), ("tile_order", C.c_void_p),
                ("depths", C.c_void_p), ("out_depth", C.c_void_p)]


class BlendBackwardOpts(C.Structure):
    """struct cugs_blend_backward_opts."""
    _fields_ = [("prezeroed", C.c_int), ("abs_grad", C.c_int), ("tile_order", C.c_void_p), ("depths", C.c_void_p),
                ("dL_ddepth_map", C.c_void_p), ("dL_dalpha", C.c_void_p), ("dL_ddepths", C.c_void_p),
                ("dL_dmeans_2d_abs", C.c_void_p)]


class LossOpts(C.Structure):
    """struct cugs_loss_opts."""
    _fields_ = [("exposure", C.c_void_p), ("mask", C.c_void_p), ("dL_dexposure", C.c_void_p), ("corrected", C.c_void_p)]


class DepthLossOpts(C.Structure):
    """struct cugs_depth_loss_opts."""
    _fields_ = [("weight", C.c_void_p), ("scale_shift", C.c_void_p), ("fit", C.c_int), ("inverse", C.c_int),
                ("min_alpha", C.c_float), ("expected", C.c_void_p)]


class NormalLossOpts(C.Structure):
    """struct cugs_normal_loss_opts."""
    _fields_ = [("weight", C.c_void_p), ("normals_out", C.c_void_p), ("cos_weight", C.c_float), ("l1_weight", C.c_float),
                ("min_alpha", C.c_float)]


class TsdfVolume(C.Structure):
    """struct cugs_tsdf_volume."""
    _fields_ = [("planes", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("color", C.c_int32),
                ("origin", C.c_float * 3), ("voxel_size", C.c_float), ("trunc", C.c_float)]


class TsdfView(C.Structure):
    """struct cugs_tsdf_view."""
    _fields_ = [("camera", Camera), ("depth_map", C.c_void_p), ("alpha", C.c_void_p), ("color", C.c_void_p),
                ("weight", C.c_void_p)]


class TsdfOpts(C.Structure):
    """struct cugs_tsdf_opts."""
    _fields_ = [("min_depth", C.c_float), ("min_alpha", C.c_float), ("max_weight", C.c_float)]


class Similarity(C.Structure):
    """struct CugsSimilarity."""
    _fields_ = [("m", C.c_float * 9), ("t", C.c_float * 3), ("log_scale", C.c_float), ("q", C.c_float * 4),
                ("d1", C.c_float * 9), ("d2", C.c_float * 25), ("d3", C.c_float * 49), ("flags", C.c_uint32)]


SIMILARITY_ROTATION_IS_IDENTITY, SIMILARITY_SCALE_IS_ONE = 1, 2         # CUGS_SIMILARITY_*
TRANSFORM_MAX_ZERO = 8                                                  # CUGS_TRANSFORM_MAX_ZERO


class BilagridDims(C.Structure):
    """struct cugs_bilagrid_dims."""
    _fields_ = [("l", C.c_int32), ("gy", C.c_int32), ("gx", C.c_int32)]


class EnvmapView(C.Structure):
    """struct cugs_envmap_view."""
    _fields_ = [("m", C.c_float * 9), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32), ("resolution", C.c_int32)]


_P = C.c_void_p
_I = C.c_int
_L = C.c_int64
_F = C.c_float
_U32 = C.c_uint32
_U64 = C.c_uint64

# name -> (restype, argtypes); must list every function of include/cugs_hip.h
SIGNATURES = {
    "cugs_version": (C.c_char_p, []),
    "cugs_error_string": (C.c_char_p, [_I]),
    "cugs_project_forward": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, C.POINTER(Camera), _F,
                                  _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "cugs_project_forward_keyed": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, C.POINTER(Camera), _F,
                                        _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cugs_project_forward_geometry": (_I, [_L, _P, _P, _P, _P, C.POINTER(Camera), _F, _P, _P, _P, _P, _P, _P, _P, _P,
                                           C.c_size_t, _P]),
    "cugs_project_forward_colour": (_I, [_L, _I, _I, _P, _P, C.POINTER(Camera), _P, _P, _P, _P]),
    "cugs_evaluate_sh": (_I, [_I, _L, _I, _P, _P, _P, _P]),
    "cugs_evaluate_sh_backward": (_I, [_I, _L, _I, _P, _P, _P, _P, _P]),
    "cugs_pack_projected": (_I, [_L, _P, _P, _P, _P, _P, _P]),
    "cugs_sort_workspace_bytes": (C.c_size_t, [_L]),
    "cugs_sort_pair_workspace_bytes": (C.c_size_t, [_L]),
    "cugs_sort_count_pairs": (_I, [_L, _P, _P, _P, _P, _I, _I, _P, C.c_size_t, C.POINTER(C.c_int64), _P]),
    "cugs_sort_count_pairs_wide": (_I, [_L, _P, _P, _P, _P, _I, _I, _P, C.c_size_t, C.POINTER(C.c_int64), _P]),
    "cugs_sort_pairs_predicted_wide": (_I, [_L, _L, _P, _P, _P, _P, _I, _I, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P,
                                            C.POINTER(C.c_int64), _P]),
    "cugs_sort_pairs": (_I, [_L, _L, _P, _P, _P, _P, _I, _I, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P]),
    "cugs_sort_pairs_predicted": (_I, [_L, _L, _P, _P, _P, _P, _I, _I, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P,
                                       C.POINTER(C.c_int64), _P]),
    "cugs_sort_pairs_predicted_keyed": (_I, [_L, _L, _P, _P, _P, _P, _I, _I, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P,
                                             C.POINTER(C.c_int64), _P]),
    "cugs_sort_pairs_predicted_keyed_ordered": (_I, [_L, _L, _P, _P, _P, _P, _I, _I, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P,
                                                     C.POINTER(C.c_int64), _P, _P]),
    "cugs_tile_order": (_I, [_I, _I, _P, _P, _P]),
    "cugs_rasterize_forward": (_I, [_I, _I, C.POINTER(C.c_float), _P, _P, _P, _P, _P, _P, _P,
                                    _P, _P, _P, _P]),
    "cugs_rasterize_forward_opts": (_I, [_I, _I, C.POINTER(C.c_float), _P, _P, _P, _P, _P, _P, _P,
                                         _P, _P, _P, C.POINTER(BlendForwardOpts), _P]),
    "cugs_blend_scores": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "cugs_blend_lift": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _P]),
    "cugs_rasterize_backward": (_I, [_I, _I, C.POINTER(C.c_float), _P, _P, _P, _P, _P, _P, _P,
                                     _P, _P, _P, _L, _P, _P, _P, _P, _P, _P]),
    "cugs_rasterize_backward_opts": (_I, [_I, _I, C.POINTER(C.c_float), _P, _P, _P, _P, _P, _P, _P,
                                          _P, _P, _P, _L, _P, _P, _P, _P, _P, C.POINTER(BlendBackwardOpts), _P]),
    "cugs_project_backward": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Camera), _F,
                                   _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "cugs_project_backward_adam": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Camera), _F, _P,
                                        C.POINTER(AdamFused), _P, _P]),
    "cugs_sh_backward_views": (_I, [_I, _L, _I, _P, _I, _P, C.POINTER(C.c_float), _P, _P]),
    "cugs_gated_colour_grad": (_I, [_L, _P, _P, _P, _P]),
    "cugs_adam_bias_correction": (None, [_F, _F, _I, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "cugs_fused_adam": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _F, _P]),
    "cugs_fused_adam_groups": (_I, [C.POINTER(AdamGroup), _I, _F, _F, _F, _F, _F, _P]),
    "cugs_fused_adam_groups_rows": (_I, [C.POINTER(AdamGroup), _I, C.POINTER(C.c_int32), _P, _L, _F, _F, _F, _F, _F, _P]),
    "cugs_loss_workspace_bytes": (C.c_size_t, [_I, _I]),
    "cugs_combined_loss": (_I, [_I, _I, _P, _P, _F, _I, _P, C.c_size_t, _P, _P, _P, _P]),
    "cugs_loss_opts_workspace_bytes": (C.c_size_t, [_I, _I]),
    "cugs_combined_loss_opts": (_I, [_I, _I, _P, _P, _F, _I, C.POINTER(LossOpts), _P, C.c_size_t, _P, _P, _P, _P]),
    "cugs_depth_loss_workspace_bytes": (C.c_size_t, [_I, _I]),
    "cugs_depth_loss": (_I, [_I, _I, _P, _P, _P, C.POINTER(DepthLossOpts), _P, C.c_size_t, _P, _P, _P, _P]),
    "cugs_normal_loss_workspace_bytes": (C.c_size_t, [_I, _I]),
    "cugs_normal_loss": (_I, [_I, _I, _F, _F, _F, _F, _P, _P, _P, C.POINTER(NormalLossOpts), _P, C.c_size_t, _P, _P, _P, _P]),
    "cugs_bilagrid_workspace_bytes": (C.c_size_t, [_I, _I, C.POINTER(BilagridDims)]),
    "cugs_bilagrid_slice": (_I, [_I, _I, C.POINTER(BilagridDims), _P, _P, _P, _P]),
    "cugs_bilagrid_slice_backward": (_I, [_I, _I, C.POINTER(BilagridDims), _P, _P, _P, _P, C.c_size_t, _P, _P, _P]),
    "cugs_bilagrid_tv": (_I, [C.POINTER(BilagridDims), _P, _F, _P, _P, _I, _P]),
    "cugs_eval_workspace_bytes": (C.c_size_t, [_I, _I]),
    "cugs_eval_metrics": (_I, [_I, _I, _P, _P, _P, _I, _P, C.c_size_t, _P, _P]),
    "cugs_densify_accumulate": (_I, [_L, _P, _P, _P, _P, _P, _P]),
    "cugs_densify_accumulate_strided": (_I, [_L, _P, _L, _P, _P, _P, _P, _P]),
    "cugs_densify_classify": (_I, [_L, _P, _P, _P, _P, _P, _F, _F, _F, _I, _F, _F, _P, _P, _P]),
    "cugs_densify_workspace_bytes": (C.c_size_t, [_L]),
    "cugs_densify_plan": (_I, [_L, _P, _P, C.c_size_t, C.POINTER(C.c_int64), _P]),
    "cugs_densify_apply": (_I, [_L, _L, _P, C.c_size_t, _P, _P, C.POINTER(DensifyArray), _I, _P]),
    "cugs_mcmc_random_bits": (_I, [_U64, _U32, _U32, _U64, _L, _P, _P]),
    "cugs_mcmc_regularization": (_I, [_L, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cugs_mcmc_inject_noise": (_I, [_L, _P, _P, _P, _F, _F, _F, _P, _U64, _U32, _P]),
    "cugs_mcmc_relocate_workspace_bytes": (C.c_size_t, [_L]),
    "cugs_mcmc_relocate": (_I, [_L, _I, _P, _P, _P, _P, _P, _F, _F, _F, _U64, _U32, C.POINTER(_P), C.POINTER(_P), _P,
                                C.c_size_t, _P, _P, _P]),
    "cugs_pose_grad_workspace_bytes": (C.c_size_t, [_L]),
    "cugs_project_backward_opts": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Camera), _F,
                                        _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(ProjectionOpts), _P]),
    "cugs_project_backward_adam_opts": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Camera), _F, _P,
                                             C.POINTER(AdamFused), _P, C.POINTER(ProjectionOpts), _P]),
    "cugs_ply_vertex_floats": (_I, [_I, _I]),
    "cugs_ply_pack": (_I, [_L, _I, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P, _P]),
    "cugs_ply_unpack": (_I, [_L, _I, _I, _P, _P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P]),
    "cugs_image_to_float": (_I, [_I, _I, _P, _I, _I, _P, _P]),
    "cugs_knn_workspace_bytes": (C.c_size_t, [_L, _I]),
    "cugs_knn_mean_distances": (_I, [_L, _I, _P, _P, _P, C.c_size_t, _I, _P]),
    "cugs_init_from_points": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "cugs_tsdf_integrate": (_I, [C.POINTER(TsdfVolume), C.POINTER(TsdfView), _I, C.POINTER(TsdfOpts), _P]),
    "cugs_mesh_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "cugs_mesh_plan": (_I, [C.POINTER(TsdfVolume), _F, _P, C.c_size_t, C.POINTER(C.c_int64), _P]),
    "cugs_mesh_emit": (_I, [C.POINTER(TsdfVolume), _P, C.c_size_t, _L, _L, _P, _P, _P, _P]),
    "cugs_similarity_init": (_I, [C.POINTER(Similarity), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double]),
    "cugs_transform_gaussians": (_I, [_L, _I, _P, _P, _P, _P, _P, C.POINTER(_P), C.POINTER(C.c_int), _I,
                                      C.POINTER(Similarity), _P]),
    "cugs_vq_workspace_bytes": (C.c_size_t, [_I, _I]),
    "cugs_vq_assign": (_I, [_L, _I, _I, _P, _L, _P, _P, _P, _P, C.c_size_t, _P]),
    "cugs_vq_update": (_I, [_L, _I, _I, _P, _L, _P, _P, _I, _P, _P, _P, C.c_size_t, _P]),
    "cugs_envmap_view_init": (_I, [C.POINTER(EnvmapView), C.POINTER(Camera), C.POINTER(C.c_double), _I]),
    "cugs_envmap_workspace_bytes": (C.c_size_t, [_I]),
    "cugs_envmap_frac_bits": (_I, [_I, _I, _F]),
    "cugs_envmap_composite": (_I, [C.POINTER(EnvmapView), _P, _P, _P, _P, _P, _P, _P]),
    "cugs_envmap_composite_backward": (_I, [C.POINTER(EnvmapView), _P, _P, _P, _P, _F, _P, C.c_size_t, _P, _P, _P, _P, _P]),
    "cugs_device_count": (_I, [C.POINTER(C.c_int)]),
}


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no fallback path: the HIP library is the implementation.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise ImportError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class CugsError(RuntimeError):
    """Non-zero return from the C ABI (the adapter's std::runtime_error, cuda_utils.cuh:12-20)."""


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib.cugs_error_string(int(code)).decode()
        raise CugsError(f"{what} failed with code {code}: {msg}")


def version() -> str:
    return lib.cugs_version().decode()
