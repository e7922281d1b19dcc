"""Per-Gaussian contribution scores and score-based pruning (not in the reference).

For every Gaussian, three statistics of its blend weight w = alpha * T over the pixels of the scored views, made by
one kernel launch per view (cugs_blend_scores: the forward blend's walk without its colour):

  weight_sum    sum of w                  Mini-Splatting's importance
  weight_max    largest w on any pixel    RadSplat's pruning rule (threshold about 0.01)
  pixel_count   pixels with w > 0         LightGaussian's hit count

and the compaction that acts on them: prune_gaussians drops the rows of a mask from the model and, when given, from
the FusedAdam moments, through the device-side plan / apply of the densifier (cugs_densify_plan / cugs_densify_apply).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import DensifyArray, check, lib
from .densification import _workspace
from .rasterizer import _ptr, _stream, _torch_check, project_gaussians, sort_gaussians
from .types import CameraInfo, GaussianModel, RenderOutput, RenderSettings

_PARAMS = ("positions", "sh_coeffs", "opacities", "rotations", "scales")


class ContributionScores:
    """The score table of `n` Gaussians on `device`: [n,4] 32-bit words {sum of w, max of w, pixel count, padding},
    zeroed.  Launches ADD to it (accumulate_contribution_scores): sums and counts add up over the views, the maximum is
    the maximum over the views; `num_views` counts the launches.  The pixel count is a uint32 and wraps at 2^32."""

    def __init__(self, n: int, device):
        self.table = torch.zeros((int(n), 4), dtype=torch.int32, device=device)
        self.num_views = 0

    @property
    def n(self) -> int:
        return int(self.table.shape[0])

    @property
    def weight_sum(self) -> torch.Tensor:
        """[N] float32, a view of word 0."""
        return self.table.view(torch.float32)[:, 0]

    @property
    def weight_max(self) -> torch.Tensor:
        """[N] float32, a view of word 1."""
        return self.table.view(torch.float32)[:, 1]

    @property
    def pixel_count(self) -> torch.Tensor:
        """[N] int64, read from the uint32 word 2."""
        return self.table[:, 2].to(torch.int64) & 0xFFFFFFFF

    def reset(self) -> None:
        self.table.zero_()
        self.num_views = 0


def _launch(scores: ContributionScores, width: int, height: int, tile_ranges, gaussian_indices, means_2d, cov_2d_inv,
            opacities_act, packed, tile_order) -> None:
    dev = scores.table.device
    if tile_order is not None:
        _torch_check(tile_order.is_contiguous() and tile_order.dtype == torch.int32 and
                     tile_order.numel() == 4 * tile_ranges.shape[0], "tile_order must be a contiguous [tiles, 4] int32 tensor")
    c = lambda t: None if t is None else t.contiguous()
    check(lib.cugs_blend_scores(int(width), int(height), _ptr(c(tile_ranges)), _ptr(c(gaussian_indices)),
                                _ptr(c(means_2d)), _ptr(c(cov_2d_inv)), _ptr(c(opacities_act)), _ptr(c(packed)),
                                _ptr(tile_order), scores.n, _ptr(scores.table), _stream(dev)), "cugs_blend_scores")
    scores.num_views += 1


def blend_scores(scores: ContributionScores, means_2d: Optional[torch.Tensor], cov_2d_inv: Optional[torch.Tensor],
                 opacities: Optional[torch.Tensor], tile_ranges: torch.Tensor, gaussian_indices: torch.Tensor,
                 img_w: int, img_h: int, packed: Optional[torch.Tensor] = None,
                 tile_order: Optional[torch.Tensor] = None) -> ContributionScores:
    """The stage function (the counterpart of rasterize_forward): one cugs_blend_scores launch on the current stream,
    from the packed records or, without them, from the three reference-layout arrays.  Adds to `scores`."""
    _torch_check(scores.table.is_cuda and tile_ranges.device == scores.table.device,
                 "blend_scores: the score table and the inputs must be on one CUDA device")
    _torch_check(packed is not None or scores.n == 0 or (means_2d is not None and cov_2d_inv is not None and
                                                         opacities is not None),
                 "blend_scores: give packed or means_2d, cov_2d_inv and opacities")
    for t in (means_2d, opacities) if packed is None else (packed,):
        _torch_check(t is None or int(t.shape[0]) == scores.n, "blend_scores: the score table has another N")
    _launch(scores, img_w, img_h, tile_ranges, gaussian_indices, means_2d, cov_2d_inv, opacities, packed, tile_order)
    return scores


def accumulate_contribution_scores(scores: ContributionScores, render_out: RenderOutput,
                                   camera: CameraInfo) -> ContributionScores:
    """Adds the view of an existing RenderOutput to `scores`: one launch from its tile_ranges, gaussian_indices, packed
    records and tile_order.  A deferred render (render(defer_count=True)) is wait()ed first, which raises
    PredictionMiss as render_backward would.  Needs no for_backward state: a training loop can score the view it has
    just rendered, an evaluation loop the views it evaluates."""
    render_out.wait()
    n = int(render_out.means_2d.shape[0])
    _torch_check(n == scores.n, f"accumulate_contribution_scores: the table holds {scores.n} Gaussians, the render {n}")
    if n == 0:
        scores.num_views += 1
        return scores
    _torch_check(render_out.means_2d.device == scores.table.device,
                 "accumulate_contribution_scores: the score table is on another device")
    _launch(scores, camera.width, camera.height, render_out.tile_ranges, render_out.gaussian_indices,
            render_out.means_2d, render_out.cov_2d_inv, render_out.opacities_act, render_out.packed,
            render_out.tile_order)
    return scores


def contribution_scores(model: GaussianModel, cameras: Sequence[CameraInfo],
                        settings: Optional[RenderSettings] = None) -> ContributionScores:
    """The scores of `model` over `cameras`, offline: per view the projection (at SH degree 0: the colour is not
    used), the plain sort and the score launch - no colour blend, no image.  One host sync per view (the sort's pair
    count)."""
    _torch_check(model.is_valid(), "GaussianModel is not valid")
    _torch_check(model.positions.is_cuda, "GaussianModel must be on CUDA device")
    settings = settings if settings is not None else RenderSettings()
    n = model.num_gaussians()
    scores = ContributionScores(n, model.positions.device)
    for cam in cameras:
        if n == 0:
            scores.num_views += 1
            continue
        proj = project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam,
                                 0, settings.scale_modifier, want_colour_gate=False)
        srt = sort_gaussians(proj.means_2d, proj.depths, proj.radii, proj.tiles_touched, cam.width, cam.height,
                             want_keys=False)
        _launch(scores, cam.width, cam.height, srt.tile_ranges, srt.gaussian_values_sorted, proj.means_2d,
                proj.cov_2d_inv, proj.opacities_act, proj.packed, None)
    return scores


def prune_gaussians(model: GaussianModel, prune_mask: torch.Tensor, optimizer=None) -> int:
    """Removes the Gaussians whose entry of `prune_mask` (bool [N], on the model's device) is set; returns how many.
    The compaction is the densifier's (cugs_densify_plan / cugs_densify_apply, flag 4 = keep on the rows that stay):
    the survivors keep their relative order - hence every depth tie of a later sort - and their bits.  The model's
    five tensors are replaced in place (new tensors), and with `optimizer` (the FusedAdam built on `model`) so are its
    moments m_ / v_, the survivors keeping theirs; its pending gradients are cleared.
    Per-Gaussian state held elsewhere is the caller's: after a prune call DensificationController.reset_accumulators
    (its three accumulators are indexed by the old rows) and rebuild whatever an MCMCController or a training loop
    keeps per Gaussian.  One host sync (the plan's counts)."""
    n = model.num_gaussians()
    dev = model.positions.device
    _torch_check(model.positions.is_cuda, "prune_gaussians: model must be on CUDA")
    _torch_check(isinstance(prune_mask, torch.Tensor) and prune_mask.dtype == torch.bool and prune_mask.dim() == 1 and
                 int(prune_mask.shape[0]) == n, f"prune_gaussians: prune_mask must be a bool tensor of shape [{n}]")
    _torch_check(prune_mask.device == dev, "prune_gaussians: prune_mask must be on the model's device")
    if n == 0:
        return 0
    flags = ((~prune_mask).to(torch.uint8) << 2).contiguous()         # bit 2: keep (cugs_densify_plan)
    ws = _workspace(dev, lib.cugs_densify_workspace_bytes(n))
    counts = (C.c_int64 * 4)()
    st = _stream(dev)
    check(lib.cugs_densify_plan(n, _ptr(flags), _ptr(ws), ws.numel(), counts, st), "cugs_densify_plan")
    n_out = int(counts[3])
    if n_out == n:
        return 0

    descs = []
    def add(src: torch.Tensor, mode: int):
        s = src.contiguous()
        d = torch.empty((n_out,) + tuple(s.shape[1:]), dtype=torch.float32, device=dev)
        descs.append((s, d, int(s.numel() // n), mode))
        return d
    new_params = {name: add(getattr(model, name), _lib.DENSIFY_COPY) for name in _PARAMS}
    new_m = new_v = None
    if optimizer is not None:
        new_m = [add(t, _lib.DENSIFY_STATE) for t in optimizer.m_]
        new_v = [add(t, _lib.DENSIFY_STATE) for t in optimizer.v_]
    arr = (DensifyArray * len(descs))()
    for i, (s, d, rf, mode) in enumerate(descs):
        arr[i].src, arr[i].dst, arr[i].row_floats, arr[i].mode = s.data_ptr(), d.data_ptr(), rf, mode
    if n_out > 0:
        check(lib.cugs_densify_apply(n, n_out, _ptr(ws), ws.numel(), C.c_void_p(0), C.c_void_p(0), arr, len(descs), st),
              "cugs_densify_apply")
    for name in _PARAMS:
        setattr(model, name, new_params[name])
    if optimizer is not None:
        optimizer.m_, optimizer.v_ = new_m, new_v
        optimizer.grads_ = [None] * optimizer.kNumGroups
    return n - n_out


def prune_by_scores(model: GaussianModel, scores: ContributionScores, min_max_weight: Optional[float] = None,
                    keep_fraction: Optional[float] = None, optimizer=None) -> int:
    """Prunes by the scores; returns the number removed.
    `min_max_weight`: drop every Gaussian whose weight_max is below it (RadSplat: about 0.01; the smallest positive
    float drops exactly those that never contributed to a scored pixel).
    `keep_fraction` (0..1): keep the round(keep_fraction * N) Gaussians of largest weight_sum (libtorch's topk) and drop
    the rest.
    With both, the union of the two prunes.  A Gaussian with weight_max == 0 - it reached no pixel of any scored view -
    is eligible under either rule: it is dropped whenever a rule is given at all, whatever topk makes of the ties at
    zero.  See prune_gaussians for what happens to the optimizer and for the state the caller owns."""
    n = model.num_gaussians()
    _torch_check(scores.n == n, f"prune_by_scores: the table holds {scores.n} Gaussians, the model {n}")
    _torch_check(min_max_weight is not None or keep_fraction is not None,
                 "prune_by_scores: give min_max_weight, keep_fraction or both")
    if n == 0:
        return 0
    _torch_check(scores.table.device == model.positions.device, "prune_by_scores: the score table is on another device")
    wmax = scores.weight_max
    mask = wmax == 0.0
    if min_max_weight is not None:
        mask = mask | (wmax < float(min_max_weight))
    if keep_fraction is not None:
        _torch_check(0.0 <= float(keep_fraction) <= 1.0, "prune_by_scores: keep_fraction must lie in [0, 1]")
        keep = int(round(float(keep_fraction) * n))
        drop = torch.ones(n, dtype=torch.bool, device=mask.device)
        if keep > 0:
            drop[scores.weight_sum.topk(keep)[1]] = False
        mask = mask | drop
    return prune_gaussians(model, mask, optimizer)
