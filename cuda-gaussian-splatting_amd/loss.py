"""Host-side mirror of the reference's loss surface (src/training/loss.hpp:21-52) over the fused HIP
kernels (csrc/loss.hip): l1_loss, ssim, ssim_loss, combined_loss - plus combined_loss_and_grad, which
returns the loss together with dL/dcolor, i.e. what trainer.cpp:214-217 obtains with clone + autograd + clone.
combined_loss_exposure (not in the reference) is the same loss behind a per-view 3x4 exposure matrix
and an optional pixel mask, both applied inside the same two kernels.  depth_loss (csrc/depth_loss.hip)
is the depth-supervision loss on render()'s depth and alpha maps, with an optional scale/shift fit of the prior;
normal_loss and depth_to_normals (csrc/normal_loss.hip) are the normal supervision on the same two maps.
Scalars come back as 0-dim device tensors (no host sync), as in the reference."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from ._lib import DepthLossOpts, LossOpts, NormalLossOpts, check, lib
from .rasterizer import _ptr, _stream, _torch_check, _workspace
from .types import CameraInfo


def _validate(img: torch.Tensor, name: str) -> None:
    """validate_image (loss.cpp:14-24)"""
    _torch_check(img.dim() == 3, f"{name} must be 3-dimensional [H, W, 3], got {img.dim()} dims")
    _torch_check(img.shape[2] == 3, f"{name} must have 3 channels, got {img.shape[2]}")
    _torch_check(img.dtype == torch.float32, f"{name} must be float32, got {img.dtype}")
    _torch_check(img.is_cuda, f"{name} must be on a CUDA device")


def _validate_pair(rendered: torch.Tensor, target: torch.Tensor) -> None:
    """validate_pair (loss.cpp:27-34)"""
    _validate(rendered, "rendered")
    _validate(target, "target")
    _torch_check(rendered.shape == target.shape,
                 f"rendered and target must have the same shape, got {tuple(rendered.shape)} vs {tuple(target.shape)}")


def _run(rendered, target, lambda_, window_size, want_map, want_grad):
    _validate_pair(rendered, target)
    _torch_check(window_size % 2 == 1, f"window_size must be odd, got {window_size}")
    _torch_check(window_size >= 3, f"window_size must be >= 3, got {window_size}")
    h, w = int(rendered.shape[0]), int(rendered.shape[1])
    dev = rendered.device
    r, t = rendered.contiguous(), target.contiguous()
    out = torch.empty(4, dtype=torch.float32, device=dev)
    smap = torch.empty((h, w), dtype=torch.float32, device=dev) if want_map else None
    grad = torch.empty((h, w, 3), dtype=torch.float32, device=dev) if want_grad else None
    ws = _workspace(dev, lib.cugs_loss_workspace_bytes(w, h), "loss")
    check(lib.cugs_combined_loss(w, h, _ptr(r), _ptr(t), float(lambda_), int(window_size), _ptr(ws), ws.numel(),
                                 _ptr(out), _ptr(smap), _ptr(grad), _stream(dev)), "cugs_combined_loss")
    return out, smap, grad


def l1_loss(rendered: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return _run(rendered, target, 0.2, 11, False, False)[0][1]


def ssim(rendered: torch.Tensor, target: torch.Tensor, window_size: int = 11) -> torch.Tensor:
    """Per-pixel SSIM map [H, W] (mean across RGB)."""
    return _run(rendered, target, 0.2, window_size, True, False)[1]


def ssim_loss(rendered: torch.Tensor, target: torch.Tensor, window_size: int = 11) -> torch.Tensor:
    return _run(rendered, target, 0.2, window_size, False, False)[0][3]


def combined_loss(rendered: torch.Tensor, target: torch.Tensor, lambda_: float = 0.2) -> torch.Tensor:
    return _run(rendered, target, lambda_, 11, False, False)[0][0]


def combined_loss_and_grad(rendered: torch.Tensor, target: torch.Tensor,
                           lambda_: float = 0.2) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, dL_dcolor [H,W,3]) in two launches: replaces clone + combined_loss + backward + clone."""
    out, _, grad = _run(rendered, target, lambda_, 11, False, True)
    return out[0], grad


class ExposureLoss(NamedTuple):
    """combined_loss_exposure's results; dL_dcolor, dL_dexposure and corrected are None when not asked for."""
    loss: torch.Tensor                       # 0-dim
    dL_dcolor: Optional[torch.Tensor]        # [H,W,3] = m A^T dL/dx'
    dL_dexposure: Optional[torch.Tensor]     # [3,4]
    l1: torch.Tensor                         # 0-dim
    ssim_mean: torch.Tensor                  # 0-dim
    corrected: Optional[torch.Tensor]        # [H,W,3] = x'


def combined_loss_exposure(rendered: torch.Tensor, target: torch.Tensor, lambda_: float = 0.2,
                           exposure: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                           want_grad: bool = True, want_corrected: bool = False,
                           window_size: int = 11) -> ExposureLoss:
    """combined_loss of x' = mask * (A @ rendered + b) against y' = mask * target, with exposure = [A | b] a float32
    [3,4] device tensor (None: the identity) and mask a float32 [H,W] device tensor of weights (None: all ones).  Both
    means stay over all 3*H*W elements, so a masked pixel counts as a perfect one.  With want_grad the result carries
    dL_dcolor (ready for render_backward) and, when an exposure is given, dL_dexposure [3,4]: twelve fixed-order fp64
    sums, the same bits from run to run.  No gradient flows to the mask or the target.  Still two launches over the
    image (plus a one-workgroup reduction for dL_dexposure) and no host sync.  With neither exposure nor mask (and no
    want_corrected) this is combined_loss_and_grad, bit for bit."""
    _validate_pair(rendered, target)
    _torch_check(window_size % 2 == 1, f"window_size must be odd, got {window_size}")
    _torch_check(window_size >= 3, f"window_size must be >= 3, got {window_size}")
    h, w = int(rendered.shape[0]), int(rendered.shape[1])
    dev = rendered.device
    if exposure is not None:
        _torch_check(tuple(exposure.shape) == (3, 4), f"exposure must be [3, 4], got {tuple(exposure.shape)}")
        _torch_check(exposure.dtype == torch.float32, f"exposure must be float32, got {exposure.dtype}")
        _torch_check(exposure.is_cuda and exposure.device == dev, "exposure must be on the images' CUDA device")
        _torch_check(exposure.is_contiguous(), "exposure must be contiguous (a row of ExposureModel.params is)")
    if mask is not None:
        _torch_check(tuple(mask.shape) == (h, w), f"mask must be [H, W] = {(h, w)}, got {tuple(mask.shape)}")
        _torch_check(mask.dtype == torch.float32, f"mask must be float32, got {mask.dtype}")
        _torch_check(mask.is_cuda and mask.device == dev, "mask must be on the images' CUDA device")
        mask = mask.contiguous()
    r, t = rendered.contiguous(), target.contiguous()
    out = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty((h, w, 3), dtype=torch.float32, device=dev) if want_grad else None
    d_exp = torch.empty((3, 4), dtype=torch.float32, device=dev) if want_grad and exposure is not None else None
    corrected = torch.empty((h, w, 3), dtype=torch.float32, device=dev) if want_corrected else None
    opts = LossOpts(exposure=_ptr(exposure), mask=_ptr(mask), dL_dexposure=_ptr(d_exp), corrected=_ptr(corrected))
    ws = _workspace(dev, lib.cugs_loss_opts_workspace_bytes(w, h), "loss")
    check(lib.cugs_combined_loss_opts(w, h, _ptr(r), _ptr(t), float(lambda_), int(window_size), C.byref(opts), _ptr(ws),
                                      ws.numel(), _ptr(out), None, _ptr(grad), _stream(dev)), "cugs_combined_loss_opts")
    return ExposureLoss(out[0], grad, d_exp, out[1], out[2], corrected)


class DepthLoss(NamedTuple):
    """depth_loss's results; the gradients and expected are None when not asked for."""
    loss: torch.Tensor                       # 0-dim
    dL_ddepth_map: Optional[torch.Tensor]    # [H,W]
    dL_dalpha: Optional[torch.Tensor]        # [H,W]
    scale_shift: torch.Tensor                # [2] = (s, b) the target was aligned with
    valid_weight: torch.Tensor               # 0-dim: sum of the weights of the valid pixels
    valid_count: torch.Tensor                # 0-dim float: number of valid pixels
    fit_ok: torch.Tensor                     # 0-dim float: 0 when a fit was asked for and rejected, else 1
    expected: Optional[torch.Tensor]         # [H,W] = x, 0 where invalid


def _validate_map(t: torch.Tensor, name: str, h: int, w: int, dev: torch.device) -> None:
    _torch_check(tuple(t.shape) == (h, w), f"{name} must be [H, W] = {(h, w)}, got {tuple(t.shape)}")
    _torch_check(t.dtype == torch.float32, f"{name} must be float32, got {t.dtype}")
    _torch_check(t.is_cuda and t.device == dev, f"{name} must be on the depth map's CUDA device")


def depth_loss(depth_map: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor,
               weight: Optional[torch.Tensor] = None, inverse: bool = False, align=None, min_alpha: float = 1e-3,
               want_grad: bool = True, want_expected: bool = False) -> DepthLoss:
    """Depth supervision (not in the reference): the L1 loss of the expected depth x = depth_map / alpha
    (inverse=True: x = alpha / depth_map, against an inverse-depth or disparity prior) against s * target + b, and its
    gradients with respect to render()'s two maps:

        d = depth_loss(out.depth_map, out.alpha, prior, align="fit")
        render_backward(dL_dcolor, out, model, cam, settings, dL_ddepth_map=d.dL_ddepth_map, dL_dalpha=d.dL_dalpha)

    All maps are float32 [H,W] on one CUDA device.  A pixel counts iff alpha > min_alpha, weight > 0 (None: all ones),
    0 < target < inf (a NaN or 0 marks "no data") and, in inverse space, depth_map > 0; elsewhere both gradients and
    `expected` are 0.  The mean is over all H*W pixels, so an invalid pixel counts as a perfect one.
    align: None for (s, b) = (1, 0); a float32 [2] device tensor (s, b), e.g. precomputed per image; or "fit" for the
    weighted least squares of the target to x over the valid pixels, solved on the device in fp64 - fit_ok is 0 and
    (s, b) = (1, 0) when fewer than two pixels are valid or the target is constant.  (s, b) is a constant in the
    gradient, as with a fit under no_grad.  Two launches (four with a fit), no host sync, no allocation beyond the
    outputs, and the same bits from run to run.  Every scalar comes back as a 0-dim device tensor."""
    _torch_check(depth_map.dim() == 2, f"depth_map must be 2-dimensional [H, W], got {depth_map.dim()} dims")
    _torch_check(depth_map.dtype == torch.float32, f"depth_map must be float32, got {depth_map.dtype}")
    _torch_check(depth_map.is_cuda, "depth_map must be on a CUDA device")
    h, w = int(depth_map.shape[0]), int(depth_map.shape[1])
    dev = depth_map.device
    _validate_map(alpha, "alpha", h, w, dev)
    _validate_map(target, "target", h, w, dev)
    if weight is not None:
        _validate_map(weight, "weight", h, w, dev)
        weight = weight.contiguous()
    _torch_check(0.0 < float(min_alpha) < float("inf"), f"min_alpha must be positive and finite, got {min_alpha}")
    fit, given = False, None
    if isinstance(align, str):
        _torch_check(align == "fit", f'align must be None, "fit" or a float32 [2] tensor, got {align!r}')
        fit = True
    elif align is not None:
        _torch_check(isinstance(align, torch.Tensor), f'align must be None, "fit" or a float32 [2] tensor, got {type(align).__name__}')
        _torch_check(tuple(align.shape) == (2,), f"align must be [2] = (s, b), got {tuple(align.shape)}")
        _torch_check(align.dtype == torch.float32, f"align must be float32, got {align.dtype}")
        _torch_check(align.is_cuda and align.device == dev, "align must be on the depth map's CUDA device")
        given = align.contiguous()
    d, a, t = depth_map.contiguous(), alpha.contiguous(), target.contiguous()
    out = torch.empty(8, dtype=torch.float32, device=dev)
    g_d = torch.empty((h, w), dtype=torch.float32, device=dev) if want_grad else None
    g_a = torch.empty((h, w), dtype=torch.float32, device=dev) if want_grad else None
    expected = torch.empty((h, w), dtype=torch.float32, device=dev) if want_expected else None
    opts = DepthLossOpts(weight=_ptr(weight), scale_shift=_ptr(given), fit=int(fit), inverse=int(bool(inverse)),
                         min_alpha=float(min_alpha), expected=_ptr(expected))
    ws = _workspace(dev, lib.cugs_depth_loss_workspace_bytes(w, h), "depth_loss")
    check(lib.cugs_depth_loss(w, h, _ptr(d), _ptr(a), _ptr(t), C.byref(opts), _ptr(ws), ws.numel(), _ptr(out), _ptr(g_d),
                              _ptr(g_a), _stream(dev)), "cugs_depth_loss")
    return DepthLoss(out[0], g_d, g_a, out[1:3], out[3], out[4], out[5], expected)


class NormalLoss(NamedTuple):
    """normal_loss's results; the gradients and normals are None when not asked for (or, the gradients, without a prior)."""
    loss: torch.Tensor                       # 0-dim
    dL_ddepth_map: Optional[torch.Tensor]    # [H,W]
    dL_dalpha: Optional[torch.Tensor]        # [H,W]
    valid_weight: torch.Tensor               # 0-dim: sum of the weights of the loss-valid pixels
    valid_count: torch.Tensor                # 0-dim float: number of loss-valid pixels
    normals: Optional[torch.Tensor]          # [3,H,W] = n^, 0 where not normal-valid


def normal_loss(depth_map: torch.Tensor, alpha: torch.Tensor, camera: CameraInfo, target: Optional[torch.Tensor] = None,
                weight: Optional[torch.Tensor] = None, cos_weight: float = 1.0, l1_weight: float = 0.0,
                min_alpha: float = 1e-3, want_grad: bool = True, want_normals: bool = False) -> NormalLoss:
    """Normal supervision from the rendered depth (not in the reference): the surface normal of the
    expected depth depth_map / alpha - back-projected through the camera's pinhole intrinsics, central differences,
    n = Py x Px normalised: the 2DGS depth_to_normal, in camera axes (x right, y down, z forward) and pointing at the
    camera - against a normal prior `target` [3,H,W] in the same axes, and the gradients to render()'s two maps:

        n = normal_loss(out.depth_map, out.alpha, cam, prior)
        render_backward(dL_dcolor, out, model, cam, settings, dL_ddepth_map=n.dL_ddepth_map, dL_dalpha=n.dL_dalpha)

    loss = mean over all H*W pixels of weight * (cos_weight * (1 - n.t) + l1_weight * |n - t|_1) on the pixels that
    count: not on the image border, alpha > min_alpha there and at the four neighbours, a normal of finite non-zero
    length, weight > 0 (None: all ones) and a prior vector of finite non-zero length (a zero or NaN vector marks "no
    data"; the prior is normalised in the kernel).  The masks are constants in the gradient; both gradients are 0 where
    a pixel takes part in no counted stencil.  target=None only computes the normal map (loss 0, no gradients).  Two
    launches, no host sync, no allocation beyond the outputs, the same bits from run to run and whatever the tiling.
    Every scalar comes back as a 0-dim device tensor."""
    _torch_check(depth_map.dim() == 2, f"depth_map must be 2-dimensional [H, W], got {depth_map.dim()} dims")
    _torch_check(depth_map.dtype == torch.float32, f"depth_map must be float32, got {depth_map.dtype}")
    _torch_check(depth_map.is_cuda, "depth_map must be on a CUDA device")
    h, w = int(depth_map.shape[0]), int(depth_map.shape[1])
    dev = depth_map.device
    _validate_map(alpha, "alpha", h, w, dev)
    _torch_check(isinstance(camera, CameraInfo), f"camera must be a CameraInfo, got {type(camera).__name__}")
    K = camera.intrinsics
    fx, fy, cx, cy = float(K.fx), float(K.fy), float(K.cx), float(K.cy)
    inf = float("inf")
    _torch_check(0.0 < fx < inf and 0.0 < fy < inf, f"camera fx, fy must be positive and finite, got {fx}, {fy}")
    _torch_check(-inf < cx < inf and -inf < cy < inf, f"camera cx, cy must be finite, got {cx}, {cy}")
    _torch_check(0.0 < float(min_alpha) < inf, f"min_alpha must be positive and finite, got {min_alpha}")
    _torch_check(0.0 <= float(cos_weight) < inf and 0.0 <= float(l1_weight) < inf,
                 f"cos_weight and l1_weight must be non-negative and finite, got {cos_weight}, {l1_weight}")
    if target is not None:
        _torch_check(tuple(target.shape) == (3, h, w), f"target must be [3, H, W] = {(3, h, w)}, got {tuple(target.shape)}")
        _torch_check(target.dtype == torch.float32, f"target must be float32, got {target.dtype}")
        _torch_check(target.is_cuda and target.device == dev, "target must be on the depth map's CUDA device")
        _torch_check(float(cos_weight) > 0.0 or float(l1_weight) > 0.0, "cos_weight and l1_weight must not both be 0")
        target = target.contiguous()
    else:
        _torch_check(weight is None, "weight needs a target")
        _torch_check(want_normals, "without a target there is only the normal map: want_normals must be True")
    if weight is not None:
        _validate_map(weight, "weight", h, w, dev)
        weight = weight.contiguous()
    d, a = depth_map.contiguous(), alpha.contiguous()
    want_grad = bool(want_grad) and target is not None
    out = torch.empty(8, dtype=torch.float32, device=dev)
    g_d = torch.empty((h, w), dtype=torch.float32, device=dev) if want_grad else None
    g_a = torch.empty((h, w), dtype=torch.float32, device=dev) if want_grad else None
    normals = torch.empty((3, h, w), dtype=torch.float32, device=dev) if want_normals else None
    opts = NormalLossOpts(weight=_ptr(weight), normals_out=_ptr(normals), cos_weight=float(cos_weight),
                          l1_weight=float(l1_weight), min_alpha=float(min_alpha))
    ws = _workspace(dev, lib.cugs_normal_loss_workspace_bytes(w, h), "normal_loss")
    check(lib.cugs_normal_loss(w, h, fx, fy, cx, cy, _ptr(d), _ptr(a), _ptr(target), C.byref(opts), _ptr(ws), ws.numel(),
                               _ptr(out), _ptr(g_d), _ptr(g_a), _stream(dev)), "cugs_normal_loss")
    return NormalLoss(out[0], g_d, g_a, out[1], out[2], normals)


def depth_to_normals(depth_map: torch.Tensor, alpha: torch.Tensor, camera: CameraInfo,
                     min_alpha: float = 1e-3) -> torch.Tensor:
    """The normal map [3,H,W] of normal_loss without a prior: what one looks at to judge the geometry (0 on the image
    border and wherever alpha <= min_alpha at the pixel or one of its four neighbours)."""
    return normal_loss(depth_map, alpha, camera, None, min_alpha=min_alpha, want_normals=True).normals
