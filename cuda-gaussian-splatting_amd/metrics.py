"""Host-side mirror of the reference's evaluation module (src/training/metrics.hpp:22-76, metrics.cpp) over
csrc/metrics.hip: compute_psnr, compute_ssim, ImageMetrics, EvalResults and evaluate - plus eval_metrics, the device row
{MSE, mean SSIM, L1 mean, max |x - y|} of one view with no host sync.  The target may be a float32 [H, W, 3] image or
the uint8 [H, W, 3] a ViewCache holds (expanded in registers, never materialised as float).  evaluate() queues every
view's render and metric kernels, fills one [V, 4] device table and reads it back ONCE (the reference blocks on two
.item() calls per view, metrics.cpp:27,45)."""
from __future__ import annotations

import json
import math
import os
import time
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from ._lib import check, lib
from .rasterizer import _ptr, _stream, _torch_check, _workspace, render
from .types import CameraInfo, GaussianModel, RenderSettings
from .views import StreamedViewCache, ViewCache, image_to_float


def _validate(rendered: torch.Tensor, target: torch.Tensor, who: str) -> None:
    """metrics.cpp:22-25, then what the kernel needs (validate_image, loss.cpp:14-24; the target may be 8-bit)."""
    _torch_check(tuple(rendered.shape) == tuple(target.shape), f"{who}: rendered and target must have same shape")
    _torch_check(rendered.dim() == 3 and rendered.shape[2] == 3, f"{who}: expected [H, W, 3] tensors")
    _torch_check(rendered.dtype == torch.float32, f"{who}: rendered must be float32, got {rendered.dtype}")
    _torch_check(target.dtype in (torch.float32, torch.uint8), f"{who}: target must be float32 or uint8, got {target.dtype}")
    _torch_check(rendered.is_cuda and target.is_cuda, f"{who}: rendered and target must be on a CUDA device")
    _torch_check(rendered.device == target.device, f"{who}: rendered and target must be on the same device")


def _eval_row(rendered, target, out, window_size: int, who: str) -> torch.Tensor:
    _validate(rendered, target, who)
    _torch_check(window_size % 2 == 1, f"window_size must be odd, got {window_size}")
    _torch_check(3 <= window_size <= 15, f"window_size must be in 3..15, got {window_size}")
    h, w = int(rendered.shape[0]), int(rendered.shape[1])
    dev = rendered.device
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=dev)
    else:
        _torch_check(out.dtype == torch.float32 and out.device == dev and out.numel() == 4 and out.is_contiguous(),
                     f"{who}: out must be a contiguous float32 [4] on the images' device")
    r, t = rendered.contiguous(), target.contiguous()
    f32 = t.dtype == torch.float32
    ws = _workspace(dev, lib.cugs_eval_workspace_bytes(w, h), "eval")
    check(lib.cugs_eval_metrics(w, h, _ptr(r), _ptr(t) if f32 else None, None if f32 else _ptr(t), int(window_size),
                                _ptr(ws), ws.numel(), _ptr(out), _stream(dev)), "cugs_eval_metrics")
    return out


def eval_metrics(rendered: torch.Tensor, target: torch.Tensor, out: Optional[torch.Tensor] = None,
                 window_size: int = 11) -> torch.Tensor:
    """Device float[4] = {MSE, mean SSIM, L1 mean, max |rendered - target|}; two launches, no host sync.  `out`: a
    contiguous float32 [4] on the same device (row v of a [V, 4] table) to write into instead of a new tensor.
    Mean SSIM and the L1 mean are the bits of combined_loss's loss_out[2] and [1]; a NaN input gives NaN."""
    return _eval_row(rendered, target, out, window_size, "eval_metrics")


def psnr_from_mse(mse) -> float:
    """metrics.cpp:27-34 in float32 arithmetic: identical images are clamped at 100 dB."""
    mse = np.float32(mse)
    if mse < np.float32(1e-10):
        return 100.0
    with np.errstate(all="ignore"):
        return float(np.float32(10.0) * np.log10(np.float32(1.0) / mse))


def compute_psnr(rendered: torch.Tensor, target: torch.Tensor) -> float:
    """PSNR = 10 log10(1 / MSE) in dB for values in [0, 1] (metrics.hpp:22-30).  Blocks on a 16-byte read-back."""
    return psnr_from_mse(_eval_row(rendered, target, None, 11, "PSNR").cpu().numpy()[0])


def compute_ssim(rendered: torch.Tensor, target: torch.Tensor) -> float:
    """Mean SSIM (metrics.hpp:32-39): the number the training log's ssim term is made of.  Blocks on a read-back."""
    return float(_eval_row(rendered, target, None, 11, "SSIM").cpu().numpy()[1])


@dataclass
class ImageMetrics:
    """metrics.hpp:42-46"""
    image_name: str = ""
    psnr: float = 0.0
    ssim: float = 0.0


def _num(v: float):
    """A JSON number; non-finite values become null, as nlohmann's dump writes them."""
    v = float(v)
    return v if math.isfinite(v) else None


@dataclass
class EvalResults:
    """metrics.hpp:49-62"""
    mean_psnr: float = 0.0
    mean_ssim: float = 0.0
    per_image: List[ImageMetrics] = field(default_factory=list)
    num_gaussians: int = 0
    sh_degree: int = 0
    eval_time_seconds: float = 0.0

    def to_json(self) -> str:
        """metrics.cpp:52-72: the reference's keys, 2-space indent, keys in nlohmann's (sorted) order."""
        j = {"mean_psnr": _num(self.mean_psnr), "mean_ssim": _num(self.mean_ssim),
             "num_gaussians": int(self.num_gaussians), "sh_degree": int(self.sh_degree),
             "eval_time_seconds": _num(self.eval_time_seconds), "num_test_images": len(self.per_image),
             "per_image": [{"image_name": im.image_name, "psnr": _num(im.psnr), "ssim": _num(im.ssim)}
                           for im in self.per_image]}
        return json.dumps(j, indent=2, sort_keys=True, ensure_ascii=False)

    def save_json(self, path) -> None:
        """metrics.cpp:78-87"""
        parent = os.path.dirname(os.fspath(path))
        if parent:
            os.makedirs(parent, exist_ok=True)
        with open(path, "w") as f:
            f.write(self.to_json() + "\n")


def _target_of(targets, v: int, w: int, h: int):
    """(tensor for the metric kernel, release callback or None): the cached 8-bit view itself when it already has the
    camera's size, else the float target at that size (the reference's resize, metrics.cpp:121-128)."""
    if isinstance(targets, (ViewCache, StreamedViewCache)):
        if targets.size(v) == (w, h):
            return targets.view_u8(v), (lambda: targets.done_reading(v))
        return targets.target(v, w, h), None
    t = targets[v]
    if t.dtype == torch.uint8 and (int(t.shape[1]), int(t.shape[0])) != (w, h):
        return image_to_float(t, w, h), None
    return t, None


def evaluate(model: GaussianModel, cameras: Sequence[CameraInfo], targets, settings: RenderSettings,
             image_names: Optional[Sequence[str]] = None) -> EvalResults:
    """metrics.cpp:93-163 on held-out views.  `targets`: a ViewCache, a StreamedViewCache (view v + 1 travels to the
    device while view v renders) or a sequence of device tensors, one per camera - uint8 [h, w, 3] (resized to the
    camera when the sizes differ) or float32 [H, W, 3].  One device-to-host copy, of the [V, 4] table, at the end."""
    num_test = len(cameras)
    if num_test == 0:                                        # metrics.cpp:98-102
        return EvalResults()
    _torch_check(len(targets) >= num_test, f"evaluate: {num_test} cameras but {len(targets)} targets")
    _torch_check(image_names is None or len(image_names) >= num_test, "evaluate: fewer image names than cameras")
    res = EvalResults(num_gaussians=int(model.num_gaussians()), sh_degree=int(settings.active_sh_degree))
    t_start = time.monotonic()
    dev = model.positions.device
    table = torch.empty((num_test, 4), dtype=torch.float32, device=dev)
    streamed = isinstance(targets, StreamedViewCache)
    if streamed:
        targets.prefetch(0)
    with torch.no_grad():
        for v, cam in enumerate(cameras):
            if streamed and v + 1 < num_test:
                targets.prefetch(v + 1)
            color = render(model, cam, settings, for_backward=False).color
            tgt, release = _target_of(targets, v, int(cam.width), int(cam.height))
            _eval_row(color, tgt, table[v], 11, "evaluate")
            if release is not None:
                release()
    rows = table.cpu().numpy()                               # the one read-back
    sum_psnr, sum_ssim = np.float32(0.0), np.float32(0.0)
    for v, cam in enumerate(cameras):
        name = image_names[v] if image_names is not None else getattr(cam, "image_name", "")
        psnr, ssim_val = psnr_from_mse(rows[v, 0]), float(rows[v, 1])
        res.per_image.append(ImageMetrics(str(name), psnr, ssim_val))
        sum_psnr = np.float32(sum_psnr + np.float32(psnr))   # float running sums in view order, metrics.cpp:143-151
        sum_ssim = np.float32(sum_ssim + np.float32(ssim_val))
    res.mean_psnr = float(sum_psnr / np.float32(num_test))
    res.mean_ssim = float(sum_ssim / np.float32(num_test))
    res.eval_time_seconds = float(np.float32(time.monotonic() - t_start))
    return res
