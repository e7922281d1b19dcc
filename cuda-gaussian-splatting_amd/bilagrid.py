"""Per-view bilateral-grid colour correction (not in the reference; DESIGN.md 4.22, csrc/bilagrid.hip): a small 3-D lattice
of 3x4 affine colour transforms per training view, indexed by pixel position and luminance, sliced per pixel with
trilinear weights - vignetting, local tone mapping and per-region white balance, where ExposureModel has one global
transform - and trained with the model under a total-variation regulariser.

The training loop, between render and render_backward:

    out = render(model, cam, settings)
    corrected = bilagrid_slice(grids.grid(view), out.color)
    loss, g = combined_loss_and_grad(corrected, target)
    back = bilagrid_slice_backward(grids.grid(view), out.color, g)
    tv, back_grid = bilagrid_tv(grids.grid(view), weight=10.0, dL_dgrid=back.dL_dgrid)     # adds to the same buffer
    render_backward(back.dL_drendered, out, model, cam, settings)
    grids.step(view, back_grid, step)

Held-out views have no grid: they are evaluated on render()'s colour as it is."""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from ._lib import AdamGroup, BilagridDims, check, lib
from .fused_adam import PositionLRConfig, position_lr
from .loss import _validate
from .rasterizer import _ptr, _stream, _torch_check, _workspace

GRID_MIN, GRID_MAX = 2, 64


def _validate_grid(grid: torch.Tensor, dev: Optional[torch.device] = None) -> BilagridDims:
    _torch_check(grid.dim() == 4 and grid.shape[0] == 12, f"grid must be [12, L, GY, GX], got {tuple(grid.shape)}")
    _torch_check(all(GRID_MIN <= int(s) <= GRID_MAX for s in grid.shape[1:]),
                 f"grid extents L, GY, GX must lie in [{GRID_MIN}, {GRID_MAX}], got {tuple(grid.shape[1:])}")
    _torch_check(grid.dtype == torch.float32, f"grid must be float32, got {grid.dtype}")
    _torch_check(grid.is_cuda, "grid must be on a CUDA device")
    _torch_check(dev is None or grid.device == dev, "grid must be on the image's CUDA device")
    _torch_check(grid.is_contiguous(), "grid must be contiguous (BilateralGridModel.grid(view) is)")
    return BilagridDims(l=int(grid.shape[1]), gy=int(grid.shape[2]), gx=int(grid.shape[3]))


def bilagrid_slice(grid: torch.Tensor, rendered: torch.Tensor) -> torch.Tensor:
    """corrected [H,W,3] = A(p) rendered(p) + b(p): the 3x4 transform [A | b] of pixel p is the trilinear sample of
    grid [12,L,GY,GX] (coefficient 4i+j = row i, column j) at (x/(W-1), y/(H-1), luma), luma = 0.299 r + 0.587 g +
    0.114 b clamped to [0, 1] - grid_sample(bilinear, align_corners=True, padding_mode="border") and the affine apply,
    in one launch.  The identity grid returns `rendered` bit for bit."""
    _validate(rendered, "rendered")
    dims = _validate_grid(grid, rendered.device)
    h, w = int(rendered.shape[0]), int(rendered.shape[1])
    r = rendered.contiguous()
    out = torch.empty_like(r)
    check(lib.cugs_bilagrid_slice(w, h, C.byref(dims), _ptr(grid), _ptr(r), _ptr(out), _stream(r.device)),
          "cugs_bilagrid_slice")
    return out


class BilagridGrad(NamedTuple):
    """bilagrid_slice_backward's results; either is None when not asked for."""
    dL_drendered: Optional[torch.Tensor]     # [H,W,3], ready for render_backward
    dL_dgrid: Optional[torch.Tensor]         # [12,L,GY,GX]


def bilagrid_slice_backward(grid: torch.Tensor, rendered: torch.Tensor, dL_dcorrected: torch.Tensor,
                            want_grid_grad: bool = True, want_image_grad: bool = True) -> BilagridGrad:
    """The gradients of bilagrid_slice from dL_dcorrected [H,W,3].  dL_drendered includes the term through the
    luminance guidance (zero where the clamp is active), as autograd through grid_sample does.  dL_dgrid is written,
    not accumulated: fixed-order partial sums over the lattice's xy-cells, combined in fp64 - no float atomics, no host
    sync, the same bits from run to run."""
    _validate(rendered, "rendered")
    _validate(dL_dcorrected, "dL_dcorrected")
    _torch_check(dL_dcorrected.shape == rendered.shape,
                 f"dL_dcorrected must have rendered's shape {tuple(rendered.shape)}, got {tuple(dL_dcorrected.shape)}")
    _torch_check(dL_dcorrected.device == rendered.device, "dL_dcorrected must be on rendered's CUDA device")
    dims = _validate_grid(grid, rendered.device)
    h, w = int(rendered.shape[0]), int(rendered.shape[1])
    dev = rendered.device
    r, g = rendered.contiguous(), dL_dcorrected.contiguous()
    d_img = torch.empty_like(r) if want_image_grad else None
    d_grid = torch.empty_like(grid) if want_grid_grad else None
    ws = _workspace(dev, lib.cugs_bilagrid_workspace_bytes(w, h, C.byref(dims)), "bilagrid") if want_grid_grad else None
    check(lib.cugs_bilagrid_slice_backward(w, h, C.byref(dims), _ptr(grid), _ptr(r), _ptr(g), _ptr(ws),
                                           0 if ws is None else ws.numel(), _ptr(d_img), _ptr(d_grid), _stream(dev)),
          "cugs_bilagrid_slice_backward")
    return BilagridGrad(d_img, d_grid)


def bilagrid_tv(grid: torch.Tensor, weight: float = 1.0,
                dL_dgrid: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(tv, dL_dgrid): tv (0-dim device tensor, no host sync) is the UNWEIGHTED total variation of the grid, the sum
    over the axes z, y, x of the mean squared forward difference; dL_dgrid receives weight * dtv/dgrid - ADDED to the
    tensor given (bilagrid_slice_backward's, so one buffer carries the whole grid gradient), or written to a new one."""
    dims = _validate_grid(grid)
    accumulate = dL_dgrid is not None
    if accumulate:
        _torch_check(dL_dgrid.shape == grid.shape and dL_dgrid.dtype == torch.float32 and dL_dgrid.device == grid.device
                     and dL_dgrid.is_contiguous(), "dL_dgrid must be a contiguous float32 tensor of the grid's shape and device")
    else:
        dL_dgrid = torch.empty_like(grid)
    tv = torch.empty(1, dtype=torch.float32, device=grid.device)
    check(lib.cugs_bilagrid_tv(C.byref(dims), _ptr(grid), float(weight), _ptr(tv), _ptr(dL_dgrid), int(accumulate),
                               _stream(grid.device)), "cugs_bilagrid_tv")
    return tv[0], dL_dgrid


class BilateralGridModel:
    """`params` [V,12,L,GY,GX], the identity [I | 0] at every vertex at the start, with Adam moments of the same shape;
    grid_shape = (GX, GY, L), gsplat's order.  Mirrors ExposureModel: step(view, ...) updates the grid of the ONE view
    trained in this iteration, with bias corrections from that view's own step count (kept on the host: no sync); a
    view that is not trained does not move and its moments do not decay.  The learning rate follows position_lr's
    log-linear schedule from lr_init to lr_final over max_steps.  Held-out views are evaluated without a grid."""

    beta1, beta2, eps = 0.9, 0.999, 1e-15         # AdamConfig's

    def __init__(self, num_views: int, device, grid_shape: Sequence[int] = (16, 16, 8), lr_init: float = 2e-3,
                 lr_final: float = 2e-5, max_steps: int = 30000):
        if num_views < 0:
            raise RuntimeError(f"BilateralGridModel: num_views must be >= 0, got {num_views}")
        if len(grid_shape) != 3 or not all(GRID_MIN <= int(s) <= GRID_MAX for s in grid_shape):
            raise RuntimeError(f"BilateralGridModel: grid_shape must be (GX, GY, L), each in [{GRID_MIN}, {GRID_MAX}], "
                               f"got {tuple(grid_shape)}")
        gx, gy, l = (int(s) for s in grid_shape)
        self.device = torch.device(device)
        eye = torch.cat([torch.eye(3, dtype=torch.float32), torch.zeros((3, 1), dtype=torch.float32)], dim=1)
        self.params = eye.reshape(1, 12, 1, 1, 1).repeat(num_views, 1, l, gy, gx).contiguous().to(self.device)
        self.m_ = torch.zeros_like(self.params)
        self.v_ = torch.zeros_like(self.params)
        self.steps_ = [0] * num_views             # per-view Adam step counts
        self.lr_config = PositionLRConfig(lr_init=lr_init, lr_final=lr_final, max_steps=max_steps)

    @property
    def num_views(self) -> int:
        return int(self.params.shape[0])

    def grid(self, view: int) -> torch.Tensor:
        """The [12,L,GY,GX] grid of `view`: a zero-copy view, to hand to bilagrid_slice."""
        return self.params[self._index(view)]

    def lr(self, step: int) -> float:
        return position_lr(step, self.lr_config)

    def step(self, view: int, dL_dgrid: torch.Tensor, step: int) -> None:
        """One Adam update of the grid of `view` from its gradient [12,L,GY,GX], at training iteration `step` (for the
        learning rate): cugs_fused_adam_groups with one group.  Stream-ordered, no host sync."""
        view = self._index(view)
        g = dL_dgrid
        n = int(self.params[view].numel())
        if not (g.is_cuda and g.device == self.params.device and g.dtype == torch.float32 and g.numel() == n):
            raise RuntimeError(f"BilateralGridModel.step: dL_dgrid must be {n} float32 values on the model's device")
        g = g.contiguous()
        self.steps_[view] += 1
        bc1, bc2 = C.c_float(), C.c_float()
        lib.cugs_adam_bias_correction(self.beta1, self.beta2, self.steps_[view], C.byref(bc1), C.byref(bc2))
        group = (AdamGroup * 1)()
        group[0].param, group[0].grad = self.params[view].data_ptr(), g.data_ptr()
        group[0].m, group[0].v = self.m_[view].data_ptr(), self.v_[view].data_ptr()
        group[0].n = n
        group[0].lr = float(self.lr(step))
        stream = C.c_void_p(torch.cuda.current_stream(self.params.device).cuda_stream)
        check(lib.cugs_fused_adam_groups(group, 1, self.beta1, self.beta2, self.eps, bc1.value, bc2.value, stream),
              "cugs_fused_adam_groups")

    def state_dict(self) -> Dict[str, object]:
        """The parameters, moments and per-view step counts, tensors as clones (the grids are too large for JSON)."""
        return {"params": self.params.clone(), "m": self.m_.clone(), "v": self.v_.clone(), "steps": list(self.steps_)}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        """Restores state_dict()'s document; the shapes must be this model's."""
        for key in ("params", "m", "v"):
            t = state[key]
            if tuple(t.shape) != tuple(self.params.shape) or t.dtype != torch.float32:
                raise RuntimeError(f"BilateralGridModel.load_state_dict: {key} must be float32 {tuple(self.params.shape)}, "
                                   f"got {t.dtype} {tuple(t.shape)}")
        steps = [int(s) for s in state["steps"]]
        if len(steps) != self.num_views:
            raise RuntimeError(f"BilateralGridModel.load_state_dict: need {self.num_views} step counts, got {len(steps)}")
        self.params.copy_(state["params"])
        self.m_.copy_(state["m"])
        self.v_.copy_(state["v"])
        self.steps_ = steps

    def _index(self, view: int) -> int:
        view = int(view)
        if not 0 <= view < self.num_views:
            raise RuntimeError(f"BilateralGridModel: view {view} out of range [0, {self.num_views})")
        return view
