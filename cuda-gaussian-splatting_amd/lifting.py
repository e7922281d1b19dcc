"""Pixel maps lifted onto Gaussians (not in the reference).

For every Gaussian g and channel c, S[g,c] = sum over the pixels p of w_g(p) * M_c(p), w = alpha * T the forward's blend
weight, made by one kernel launch per view and map (cugs_blend_lift: the weighted form of the score kernel), and what is
built on that sum:

  lift_pixel_maps / lift_maps   the sums themselves, of float maps with 1..4 channels or of a label image's indicators
  error_scores                  E_g = max (or sum) over views of sum_p w_g(p) err(p): error-based densification
                                (DensificationController.accumulate_error_scores takes one view's scores)
  vote_labels                   argmax_l sum_views sum_p w_g(p) [label(p) == l]: a 2-D segmentation lifted to 3-D
  select_gaussians              keeps the rows of a mask (an object extracted by its voted label)

No gradients flow through the lift.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from ._lib import check, lib
from .importance import prune_gaussians
from .rasterizer import _ptr, _stream, _torch_check, project_gaussians, sort_gaussians
from .types import CameraInfo, GaussianModel, RenderOutput, RenderSettings

MAX_CHANNELS = 4


class LiftedMaps:
    """The table of `n` Gaussians on `device`: [n,4] float32, zeroed, of which launches ADD to words 0..channels-1 of a
    row (the others are never written).  `sums` is the [n,channels] view of it; `num_views` counts the launches."""

    def __init__(self, n: int, device, channels: int = 1):
        _torch_check(1 <= int(channels) <= MAX_CHANNELS, f"LiftedMaps: channels must be 1..{MAX_CHANNELS}")
        self.table = torch.zeros((int(n), 4), dtype=torch.float32, device=device)
        self.channels = int(channels)
        self.num_views = 0

    @property
    def n(self) -> int:
        return int(self.table.shape[0])

    @property
    def sums(self) -> torch.Tensor:
        """[N,channels] float32, a view of the table."""
        return self.table[:, :self.channels]

    def reset(self) -> None:
        self.table.zero_()
        self.num_views = 0


def _map_args(lifted: LiftedMaps, width: int, height: int, maps, labels, what: str):
    """The validated, contiguous map of one launch: (maps or None, labels or None)."""
    _torch_check((maps is None) != (labels is None), f"{what}: give exactly one of maps and labels")
    dev = lifted.table.device
    if maps is not None:
        _torch_check(isinstance(maps, torch.Tensor) and maps.device == dev and maps.dtype == torch.float32,
                     f"{what}: maps must be a float32 tensor on the table's device")
        shape = tuple(maps.shape)
        ok = shape == (height, width, lifted.channels) or (lifted.channels == 1 and shape == (height, width))
        _torch_check(ok, f"{what}: maps must be [{height}, {width}, {lifted.channels}], got {list(shape)}")
        return maps.contiguous(), None
    _torch_check(isinstance(labels, torch.Tensor) and labels.device == dev and labels.dtype == torch.int32,
                 f"{what}: labels must be an int32 tensor on the table's device")
    _torch_check(tuple(labels.shape) == (height, width), f"{what}: labels must be [{height}, {width}]")
    return None, labels.contiguous()


def _launch(lifted: LiftedMaps, width: int, height: int, tile_ranges, gaussian_indices, means_2d, cov_2d_inv,
            opacities_act, packed, tile_order, maps, labels, label_base: int) -> None:
    dev = lifted.table.device
    if tile_order is not None:
        _torch_check(tile_order.is_contiguous() and tile_order.dtype == torch.int32 and
                     tile_order.numel() == 4 * tile_ranges.shape[0], "tile_order must be a contiguous [tiles, 4] int32 tensor")
    c = lambda t: None if t is None else t.contiguous()
    check(lib.cugs_blend_lift(int(width), int(height), _ptr(c(tile_ranges)), _ptr(c(gaussian_indices)),
                              _ptr(c(means_2d)), _ptr(c(cov_2d_inv)), _ptr(c(opacities_act)), _ptr(c(packed)),
                              _ptr(tile_order), lifted.n, _ptr(maps), _ptr(labels), lifted.channels, int(label_base),
                              _ptr(lifted.table), _stream(dev)), "cugs_blend_lift")
    lifted.num_views += 1


def blend_lift(lifted: LiftedMaps, means_2d: Optional[torch.Tensor], cov_2d_inv: Optional[torch.Tensor],
               opacities: Optional[torch.Tensor], tile_ranges: torch.Tensor, gaussian_indices: torch.Tensor,
               img_w: int, img_h: int, maps: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
               label_base: int = 0, packed: Optional[torch.Tensor] = None,
               tile_order: Optional[torch.Tensor] = None) -> LiftedMaps:
    """The stage function (the counterpart of blend_scores): one cugs_blend_lift launch on the current stream, from the
    packed records or, without them, from the three reference-layout arrays.  `maps` is [H,W,C] float32 (or [H,W] for
    C = 1), `labels` [H,W] int32 with channel c the indicator of label_base + c.  Adds to `lifted`."""
    _torch_check(lifted.table.is_cuda and tile_ranges.device == lifted.table.device,
                 "blend_lift: the table and the inputs must be on one CUDA device")
    _torch_check(packed is not None or lifted.n == 0 or (means_2d is not None and cov_2d_inv is not None and
                                                         opacities is not None),
                 "blend_lift: give packed or means_2d, cov_2d_inv and opacities")
    for t in (means_2d, opacities) if packed is None else (packed,):
        _torch_check(t is None or int(t.shape[0]) == lifted.n, "blend_lift: the table has another N")
    maps, labels = _map_args(lifted, int(img_w), int(img_h), maps, labels, "blend_lift")
    _launch(lifted, img_w, img_h, tile_ranges, gaussian_indices, means_2d, cov_2d_inv, opacities, packed, tile_order,
            maps, labels, label_base)
    return lifted


def lift_pixel_maps(lifted: LiftedMaps, render_out: RenderOutput, camera: CameraInfo,
                    maps: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                    label_base: int = 0) -> LiftedMaps:
    """Adds the view of an existing RenderOutput to `lifted`: one launch from its tile_ranges, gaussian_indices, packed
    records and tile_order.  A deferred render (render(defer_count=True)) is wait()ed first.  Needs no for_backward
    state: a training loop can lift the error image of the view it has just rendered."""
    render_out.wait()
    n = int(render_out.means_2d.shape[0])
    _torch_check(n == lifted.n, f"lift_pixel_maps: the table holds {lifted.n} Gaussians, the render {n}")
    maps, labels = _map_args(lifted, camera.width, camera.height, maps, labels, "lift_pixel_maps")
    if n == 0:
        lifted.num_views += 1
        return lifted
    _torch_check(render_out.means_2d.device == lifted.table.device, "lift_pixel_maps: the table is on another device")
    _launch(lifted, camera.width, camera.height, render_out.tile_ranges, render_out.gaussian_indices,
            render_out.means_2d, render_out.cov_2d_inv, render_out.opacities_act, render_out.packed,
            render_out.tile_order, maps, labels, label_base)
    return lifted


def _sorted_view(model: GaussianModel, cam: CameraInfo, settings: RenderSettings):
    """Projection at SH degree 0 (the colour is not used) and the plain sort: one host sync (the pair count)."""
    proj = project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam,
                             0, settings.scale_modifier, want_colour_gate=False)
    srt = sort_gaussians(proj.means_2d, proj.depths, proj.radii, proj.tiles_touched, cam.width, cam.height,
                         want_keys=False)
    return proj, srt


def _launch_sorted(lifted: LiftedMaps, cam: CameraInfo, proj, srt, maps, labels, label_base: int) -> None:
    _launch(lifted, cam.width, cam.height, srt.tile_ranges, srt.gaussian_values_sorted, proj.means_2d, proj.cov_2d_inv,
            proj.opacities_act, proj.packed, None, maps, labels, label_base)


def _check_model(model: GaussianModel, cameras, per_view, what: str) -> None:
    _torch_check(model.is_valid(), "GaussianModel is not valid")
    _torch_check(model.positions.is_cuda, "GaussianModel must be on CUDA device")
    _torch_check(len(per_view) == len(cameras), f"{what}: one map per camera")


def lift_maps(model: GaussianModel, cameras: Sequence[CameraInfo], maps_per_view: Sequence[torch.Tensor],
              settings: Optional[RenderSettings] = None, channels: Optional[int] = None) -> LiftedMaps:
    """The sums of `model` over `cameras`, offline, as contribution_scores: per view the projection at SH degree 0, the
    plain sort and the lift launch of maps_per_view[i] - no colour blend, no image.  `channels` defaults to the first
    map's (1 for an [H,W] map)."""
    _check_model(model, cameras, maps_per_view, "lift_maps")
    settings = settings if settings is not None else RenderSettings()
    if channels is None:
        channels = 1 if len(maps_per_view) == 0 or maps_per_view[0].dim() == 2 else int(maps_per_view[0].shape[2])
    n = model.num_gaussians()
    lifted = LiftedMaps(n, model.positions.device, channels)
    for cam, m in zip(cameras, maps_per_view):
        m, _ = _map_args(lifted, cam.width, cam.height, m, None, "lift_maps")
        if n == 0:
            lifted.num_views += 1
            continue
        proj, srt = _sorted_view(model, cam, settings)
        _launch_sorted(lifted, cam, proj, srt, m, None, 0)
    return lifted


def vote_labels(model: GaussianModel, cameras: Sequence[CameraInfo], label_maps: Sequence[torch.Tensor],
                num_labels: int, settings: Optional[RenderSettings] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Lifts 2-D label images [H,W] int32 with labels 0..num_labels-1 to the Gaussians: votes[g,l] = sum over the
    views and pixels of w_g(p) [label(p) == l], labels[g] = argmax_l votes[g,l] (the first maximum on a tie), -1 where
    a Gaussian collected no vote.  A pixel whose label is outside 0..num_labels-1 votes for nothing.  Per view one
    projection and sort feed ceil(num_labels / 4) launches with label_base = 0, 4, 8, ...
    Returns (labels [N] int64, votes [N,num_labels] float32)."""
    _check_model(model, cameras, label_maps, "vote_labels")
    num_labels = int(num_labels)
    _torch_check(num_labels >= 1, "vote_labels: num_labels must be positive")
    settings = settings if settings is not None else RenderSettings()
    n = model.num_gaussians()
    dev = model.positions.device
    windows = [LiftedMaps(n, dev, min(MAX_CHANNELS, num_labels - base)) for base in range(0, num_labels, MAX_CHANNELS)]
    for cam, lab in zip(cameras, label_maps):
        _, lab = _map_args(windows[0], cam.width, cam.height, None, lab, "vote_labels")
        if n == 0:
            continue
        proj, srt = _sorted_view(model, cam, settings)
        for k, win in enumerate(windows):
            _launch_sorted(win, cam, proj, srt, None, lab, k * MAX_CHANNELS)
    votes = torch.cat([win.sums for win in windows], dim=1)
    labels = votes.argmax(dim=1)
    labels = torch.where(votes.gather(1, labels[:, None])[:, 0] > 0.0, labels, torch.full_like(labels, -1))
    return labels, votes


def error_scores(model: GaussianModel, cameras: Sequence[CameraInfo], error_maps: Sequence[torch.Tensor],
                 settings: Optional[RenderSettings] = None, reduce: str = "max") -> torch.Tensor:
    """Per-Gaussian error scores [N] float32 from per-view error images [H,W] float32: per view E_g = sum_p w_g(p) err(p)
    into a scratch table, the views combined by torch.maximum (reduce="max": the rule of "Revising Densification in
    Gaussian Splatting") or by addition (reduce="sum")."""
    _check_model(model, cameras, error_maps, "error_scores")
    _torch_check(reduce in ("max", "sum"), 'error_scores: reduce must be "max" or "sum"')
    settings = settings if settings is not None else RenderSettings()
    n = model.num_gaussians()
    scratch = LiftedMaps(n, model.positions.device, 1)
    out = torch.zeros(n, dtype=torch.float32, device=model.positions.device)
    for cam, err in zip(cameras, error_maps):
        err, _ = _map_args(scratch, cam.width, cam.height, err, None, "error_scores")
        if n == 0:
            continue
        proj, srt = _sorted_view(model, cam, settings)
        if reduce == "max":
            scratch.reset()
        _launch_sorted(scratch, cam, proj, srt, err, None, 0)
        if reduce == "max":
            torch.maximum(out, scratch.sums[:, 0], out=out)
    if reduce == "sum":
        out.copy_(scratch.sums[:, 0])
    return out


def select_gaussians(model: GaussianModel, keep_mask: torch.Tensor, optimizer=None) -> int:
    """The complement of prune_gaussians: keeps the Gaussians whose entry of `keep_mask` (bool [N], on the model's
    device) is set and removes the others, with prune_gaussians' guarantees (order and bits of the survivors, the
    FusedAdam moments when `optimizer` is given).  Returns the number kept."""
    _torch_check(isinstance(keep_mask, torch.Tensor) and keep_mask.dtype == torch.bool,
                 "select_gaussians: keep_mask must be a bool tensor")
    prune_gaussians(model, ~keep_mask, optimizer)
    return model.num_gaussians()
