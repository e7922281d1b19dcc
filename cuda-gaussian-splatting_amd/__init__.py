"""MI355X-native differentiable Gaussian-splat rasterizer + fused Adam.

A drop-in for the hot path of Artemarius/cuda-gaussian-splatting: hand-written HIP for gfx950
behind a C ABI (include/cugs_hip.h, built to libcugs_hip.so), with this package as the thin
host-side mirror of the reference's operator surface (namespace cugs).  Importing it loads the
shared library and raises if it is missing: there is no fallback path.

The directory is named after the reference repository (cuda-gaussian-splatting_amd), which is
not a Python identifier; load it under the module name `cugs_amd` via __graft_entry__.load_package().
"""
from ._lib import CugsError, LIB_PATH, version  # noqa: F401  (loads libcugs_hip.so or raises)
from .types import (BackwardOutput, CameraInfo, CameraIntrinsics, ForwardOutput, GaussianModel,  # noqa: F401
                    PredictionMiss, ProjectionBackwardOutput, ProjectionOutput, RasterizeBackwardOutput, RenderOutput,
                    RenderSettings, SortingOutput, K_MAX_SH_DEGREE, K_TILE_SIZE, sh_coeff_count)
from .rasterizer import (evaluate_sh_backward_cuda, evaluate_sh_cuda, project_backward,  # noqa: F401
                         project_gaussians, rasterize_backward, rasterize_forward, render, render_backward,
                         sh_backward_views, sort_gaussians)
from .fused_adam import (AdamConfig, FusedAdam, ParamGroup, PositionLRConfig,  # noqa: F401
                         active_sh_degree_for_step, lr_defaults, position_lr)
from .loss import (DepthLoss, ExposureLoss, NormalLoss, combined_loss, combined_loss_and_grad,  # noqa: F401
                   combined_loss_exposure, depth_loss, depth_to_normals, l1_loss, normal_loss, ssim, ssim_loss)
from .exposure import ExposureModel  # noqa: F401
from .bilagrid import (BilagridGrad, BilateralGridModel, bilagrid_slice, bilagrid_slice_backward,  # noqa: F401
                       bilagrid_tv)
from .envmap import (EnvGrad, EnvironmentMap, composite_background, composite_background_backward,  # noqa: F401
                     composite_environment, composite_environment_backward, envmap_frac_bits,
                     render_with_environment)
from .densification import DensificationConfig, DensificationController, DensificationStats  # noqa: F401
from .mcmc import MCMCConfig, MCMCController, MCMCStats  # noqa: F401
from .gaussian_init import init_gaussians_from_sparse, knn_mean_distances  # noqa: F401
from .pose import apply_se3, se3_exp, viewmat_grad_to_se3  # noqa: F401
from . import pose  # noqa: F401
from .ply_io import read_gaussian_ply, restore_optimizer, write_gaussian_ply  # noqa: F401
from .views import StreamedViewCache, ViewCache, image_to_float, load_image_resized, load_image_u8  # noqa: F401
from .metrics import EvalResults, ImageMetrics, compute_psnr, compute_ssim, eval_metrics, evaluate  # noqa: F401
from .importance import (ContributionScores, accumulate_contribution_scores, blend_scores,  # noqa: F401
                         contribution_scores, prune_by_scores, prune_gaussians)
from .lifting import (LiftedMaps, blend_lift, error_scores, lift_maps, lift_pixel_maps,  # noqa: F401
                      select_gaussians, vote_labels)
from .transform import (Similarity, merge_gaussians, sh_rotation_matrices, similarity_from_cameras,  # noqa: F401
                        transform_camera, transform_cameras, transform_gaussians)
from .compress import (CompressedGaussians, compress_gaussians, decompress_gaussians, nbytes,  # noqa: F401
                       read_compressed, vq_assign, vq_fit, vq_frac_bits, vq_update, write_compressed)
from .mesh import Mesh, TSDFView, TSDFVolume, extract_mesh, write_mesh_ply  # noqa: F401
from . import parallel, scene  # noqa: F401
