"""Environment-map background (not in the reference; DESIGN.md 4.28, csrc/envmap.hip): the pixels the Gaussians leave
open show a learnable octahedral sky map indexed by ray direction instead of one constant colour, so the optimiser no
longer explains the sky with far, huge, semi-transparent splats.  No render kernel changes: the model is rendered on
background 0 (the blend then leaves color = C), one pass composites I = C + T B(p), and the gradient reaches the
Gaussians through render_backward's dL_dalpha = -sum_c g_c B_c.

The training step, between render and render_backward:

    image, out = render_with_environment(model, cam, settings, env)            # settings.background == 0
    loss, g = combined_loss_and_grad(image, target)
    back = composite_environment_backward(g, out, cam, env, grad_bound=4.0 / (3 * cam.height * cam.width))
    render_backward(g, out, model, cam, settings, dL_dalpha=back.dL_dalpha); env.step(back.dL_denv, step)

The image-background routes (composite_background, composite_background_backward) do the same for a caller's own
[H,W,3] background: random, a fixed photograph, or a per-view learned image."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import AdamGroup, EnvmapView, check, lib
from .fused_adam import PositionLRConfig, position_lr
from .loss import _validate
from .rasterizer import _ptr, _stream, _torch_check, _workspace, render
from .types import CameraInfo, GaussianModel, RenderOutput, RenderSettings

RES_MIN, RES_MAX = 4, 2048


def _check_resolution(r: int) -> int:
    r = int(r)
    _torch_check(RES_MIN <= r <= RES_MAX and r & (r - 1) == 0,
                 f"the environment map's resolution must be a power of two in [{RES_MIN}, {RES_MAX}], got {r}")
    return r


def envmap_frac_bits(height: int, width: int, grad_bound: float = 1.0) -> int:
    """The fraction bits F of the map gradient's fixed-point sums (cugs_envmap_frac_bits): with 2^e the smallest power
    of two >= grad_bound and 4 H W < 2^q, F = 61 - q - e - no sum can overflow while every share stays within the bound."""
    f = int(lib.cugs_envmap_frac_bits(int(width), int(height), float(grad_bound)))
    if f < 0:
        raise ValueError(f"envmap_frac_bits: bad size {height} x {width} or grad_bound {grad_bound!r} "
                         "(finite, in [2^-60, 2^24])")
    return f


class EnvironmentMap:
    """`texture` [3,R,R] float32: one octahedral map of the whole sphere of directions, R a power of two in [4, 2048].
    Texel (i, j) of channel c is texture[c, j, i]; the centre of the map is the +z axis of the map's frame, the four
    corners its -z axis.  `orientation` (3x3, world axes to map axes, default identity) turns the world into that frame:
    a scene whose up axis is -y puts the zenith at the centre with [[1,0,0],[0,0,1],[0,-1,0]].
    step() is one Adam update of the whole texture through the fused Adam kernel, moments held inside, as
    ExposureModel.step; a texel no ray has reached has zero gradient and zero moments and keeps its bits."""

    beta1, beta2, eps = 0.9, 0.999, 1e-15         # AdamConfig's

    def __init__(self, resolution: int = 256, device="cuda", init_color: Sequence[float] = (0.0, 0.0, 0.0),
                 orientation=None, lr_init: float = 0.01, lr_final: float = 0.001, max_steps: int = 30000):
        r = _check_resolution(resolution)
        self.device = torch.device(device)
        _torch_check(len(init_color) == 3, "init_color must be three floats")
        col = torch.tensor([float(c) for c in init_color], dtype=torch.float32).reshape(3, 1, 1)
        self.texture = col.expand(3, r, r).contiguous().to(self.device)
        self.m_ = torch.zeros_like(self.texture)
        self.v_ = torch.zeros_like(self.texture)
        self.steps_ = 0
        o = np.eye(3) if orientation is None else np.array(orientation, dtype=np.float64)
        if o.shape != (3, 3) or not np.isfinite(o).all():
            raise RuntimeError("EnvironmentMap: orientation must be a finite 3x3 matrix")
        self.orientation = np.ascontiguousarray(o, dtype=np.float64)
        self.lr_config = PositionLRConfig(lr_init=lr_init, lr_final=lr_final, max_steps=max_steps)

    @property
    def resolution(self) -> int:
        return int(self.texture.shape[1])

    def view(self, camera: CameraInfo) -> EnvmapView:
        """The per-view block of the kernels: M = orientation R^T rounded once to float32, the intrinsics, the sizes."""
        _validate_texture(self.texture)
        v = EnvmapView()
        cam = camera.to_abi()
        o = self.orientation.ctypes.data_as(C.POINTER(C.c_double))
        code = lib.cugs_envmap_view_init(C.byref(v), C.byref(cam), o, self.resolution)
        _torch_check(code == 0, "EnvironmentMap: the camera needs a positive size, finite positive fx, fy and finite cx, "
                                "cy and rotation")
        return v

    def sample(self, camera: CameraInfo) -> torch.Tensor:
        """B [H,W,3]: the map seen through `camera`, the background composite_environment blends in."""
        v = self.view(camera)
        out = torch.empty((camera.height, camera.width, 3), dtype=torch.float32, device=self.texture.device)
        check(lib.cugs_envmap_composite(C.byref(v), _ptr(self.texture), None, None, None, None, _ptr(out),
                                        _stream(out.device)), "cugs_envmap_composite")
        return out

    def lr(self, step: int) -> float:
        return position_lr(step, self.lr_config)

    def step(self, dL_denv: torch.Tensor, step: int) -> None:
        """One Adam update of the texture from its gradient [3,R,R], at training iteration `step` (for the learning
        rate): cugs_fused_adam_groups with one group.  Stream-ordered, no host sync."""
        g = dL_denv
        if not (g.is_cuda and g.device == self.texture.device and g.dtype == torch.float32
                and tuple(g.shape) == tuple(self.texture.shape)):
            raise RuntimeError("EnvironmentMap.step: dL_denv must be a float32 tensor of the texture's shape and device")
        g = g.contiguous()
        self.steps_ += 1
        bc1, bc2 = C.c_float(), C.c_float()
        lib.cugs_adam_bias_correction(self.beta1, self.beta2, self.steps_, C.byref(bc1), C.byref(bc2))
        group = (AdamGroup * 1)()
        group[0].param, group[0].grad = self.texture.data_ptr(), g.data_ptr()
        group[0].m, group[0].v = self.m_.data_ptr(), self.v_.data_ptr()
        group[0].n = self.texture.numel()
        group[0].lr = float(self.lr(step))
        check(lib.cugs_fused_adam_groups(group, 1, self.beta1, self.beta2, self.eps, bc1.value, bc2.value,
                                         _stream(self.texture.device)), "cugs_fused_adam_groups")

    def save(self, path) -> None:
        """An uncompressed .npz with `texture` [3,R,R] float32 and `orientation` [3,3] float64 (one device-to-host copy).
        The moments are not stored."""
        with open(path, "wb") as f:
            np.savez(f, texture=self.texture.detach().cpu().numpy(), orientation=self.orientation)

    @classmethod
    def load(cls, path, device, **kwargs) -> "EnvironmentMap":
        """The map of save()'s file; fresh moments and step count."""
        with np.load(path) as doc:
            tex, o = np.asarray(doc["texture"]), np.asarray(doc["orientation"])
        if tex.ndim != 3 or tex.shape[0] != 3 or tex.shape[1] != tex.shape[2] or tex.dtype != np.float32:
            raise RuntimeError(f"EnvironmentMap.load: texture must be float32 [3,R,R], got {tex.dtype} {tex.shape}")
        env = cls(int(tex.shape[1]), device, orientation=o, **kwargs)
        env.texture.copy_(torch.from_numpy(np.ascontiguousarray(tex)).to(env.device))
        return env


def _validate_texture(tex: torch.Tensor, dev: Optional[torch.device] = None) -> None:
    _torch_check(tex.dim() == 3 and tex.shape[0] == 3 and tex.shape[1] == tex.shape[2],
                 f"the environment map must be [3, R, R], got {tuple(tex.shape)}")
    _check_resolution(tex.shape[1])
    _torch_check(tex.dtype == torch.float32 and tex.is_cuda and tex.is_contiguous(),
                 "the environment map must be a contiguous float32 tensor on a CUDA device")
    _torch_check(dev is None or tex.device == dev, "the environment map must be on the image's CUDA device")


def _require_zero_background(settings: RenderSettings, what: str) -> None:
    _torch_check(all(float(b) == 0.0 for b in settings.background),
                 f"{what}: the render must be made on background (0, 0, 0) - the composite adds the background itself - "
                 f"got settings.background = {list(settings.background)}")


def _validate_pair(color: torch.Tensor, final_T: torch.Tensor, what: str) -> Tuple[int, int]:
    _validate(color, what)
    h, w = int(color.shape[0]), int(color.shape[1])
    _torch_check(final_T is not None and final_T.is_cuda and final_T.device == color.device
                 and final_T.dtype == torch.float32 and tuple(final_T.shape) == (h, w),
                 f"final_T must be a float32 [H, W] = [{h}, {w}] tensor on {what}'s device")
    return h, w


def _image_view(h: int, w: int) -> EnvmapView:
    v = EnvmapView()
    v.width, v.height = w, h
    return v


def composite_environment(render_out: RenderOutput, camera: CameraInfo, env: EnvironmentMap,
                          settings: Optional[RenderSettings] = None) -> torch.Tensor:
    """image [H,W,3] = color + final_T * env.sample(camera), one launch (the multiply-add is the forward blend's own
    fmaf(T, bg, C): a uniform map of colour c gives render(background=c) bit for bit).  `render_out` must come from a
    render on background 0; pass `settings` to have that checked (render_with_environment does)."""
    if settings is not None:
        _require_zero_background(settings, "composite_environment")
    h, w = _validate_pair(render_out.color, render_out.final_T, "render_out.color")
    _torch_check((h, w) == (camera.height, camera.width), "render_out was not made with this camera's image size")
    _validate_texture(env.texture, render_out.color.device)
    v = env.view(camera)
    c, t = render_out.color.contiguous(), render_out.final_T.contiguous()
    out = torch.empty_like(c)
    check(lib.cugs_envmap_composite(C.byref(v), _ptr(env.texture), None, _ptr(c), _ptr(t), _ptr(out), None,
                                    _stream(c.device)), "cugs_envmap_composite")
    return out


class EnvGrad(NamedTuple):
    """composite_environment_backward's results."""
    dL_dalpha: torch.Tensor                  # [H,W], for render_backward(dL_dalpha=...)
    dL_denv: Optional[torch.Tensor]          # [3,R,R], for EnvironmentMap.step
    clamped: Optional[torch.Tensor]          # 0-dim int32 on the device: 1 if a share exceeded grad_bound (read or ignore)


def composite_environment_backward(dL_dimage: torch.Tensor, render_out: RenderOutput, camera: CameraInfo,
                                   env: EnvironmentMap, grad_bound: float = 1.0, want_env_grad: bool = True,
                                   settings: Optional[RenderSettings] = None) -> EnvGrad:
    """The gradients of composite_environment from dL_dimage [H,W,3].  Pass dL_dimage on to render_backward as dL_dcolor
    (dI/dC = 1) and dL_dalpha [H,W] = -sum_c g_c B_c as its dL_dalpha; dL_denv goes to env.step.

    dL_denv is summed in 64-bit fixed point through integer atomics and converted once: the same bytes on every run, no
    float atomics, no host sync.  `grad_bound` bounds |T g_c| of one pixel (each tap's share is at most that); it is
    rounded up to a power of two and fixes the scale (envmap_frac_bits).  The default 1.0 suits a sum-reduced loss on
    images in [0, 1]; a mean-reduced loss (combined_loss_and_grad) can pass something near 4 / (3 H W) and keep more
    fraction bits - at 1080p the default still leaves 2^-38 per share.  A share beyond the bound is clamped to it and sets
    `clamped`, a device word the caller may read (a sync) or ignore.

    The render must carry the alpha gradient: render_backward takes dL_dalpha on the plain and fused routes from a
    RenderOutput that still has its per-Gaussian depths and final_T (every render() has); it is refused with the
    data-parallel arguments."""
    if settings is not None:
        _require_zero_background(settings, "composite_environment_backward")
    _validate(dL_dimage, "dL_dimage")
    _torch_check(render_out.final_T is not None and render_out.depths is not None,
                 "composite_environment_backward: this RenderOutput cannot carry dL_dalpha through render_backward - "
                 "it needs final_T and the per-Gaussian depths of render()")
    h, w = _validate_pair(dL_dimage, render_out.final_T, "dL_dimage")
    _torch_check((h, w) == (camera.height, camera.width), "dL_dimage does not have this camera's image size")
    _validate_texture(env.texture, dL_dimage.device)
    dev = dL_dimage.device
    v = env.view(camera)
    g, t = dL_dimage.contiguous(), render_out.final_T.contiguous()
    d_alpha = torch.empty((h, w), dtype=torch.float32, device=dev)
    d_env = clamped = ws = None
    if want_env_grad:
        envmap_frac_bits(h, w, grad_bound)                           # raises for a bad bound
        d_env = torch.empty_like(env.texture)
        clamped = torch.empty((), dtype=torch.int32, device=dev)
        ws = _workspace(dev, lib.cugs_envmap_workspace_bytes(env.resolution), "envmap")
    check(lib.cugs_envmap_composite_backward(C.byref(v), _ptr(env.texture), None, _ptr(g), _ptr(t), float(grad_bound),
                                             _ptr(ws), 0 if ws is None else ws.numel(), _ptr(d_alpha), _ptr(d_env), None,
                                             _ptr(clamped), _stream(dev)), "cugs_envmap_composite_backward")
    return EnvGrad(d_alpha, d_env, clamped)


def composite_background(color: torch.Tensor, final_T: torch.Tensor, background: torch.Tensor) -> torch.Tensor:
    """image [H,W,3] = color + final_T * background for a caller's background image [H,W,3] (color from a render on
    background 0): fmaf(T, bg, C) per element, one launch."""
    h, w = _validate_pair(color, final_T, "color")
    _validate(background, "background")
    _torch_check(background.shape == color.shape and background.device == color.device,
                 f"background must have color's shape {tuple(color.shape)} and device")
    v = _image_view(h, w)
    c, t, b = color.contiguous(), final_T.contiguous(), background.contiguous()
    out = torch.empty_like(c)
    check(lib.cugs_envmap_composite(C.byref(v), None, _ptr(b), _ptr(c), _ptr(t), _ptr(out), None, _stream(c.device)),
          "cugs_envmap_composite")
    return out


def composite_background_backward(dL_dimage: torch.Tensor, final_T: torch.Tensor, background: torch.Tensor,
                                  want_background_grad: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(dL_dalpha [H,W], dL_dbackground [H,W,3]) of composite_background: -sum_c g_c bg_c and T g.  dL_dimage itself is
    dL_dcolor."""
    h, w = _validate_pair(dL_dimage, final_T, "dL_dimage")
    _validate(background, "background")
    _torch_check(background.shape == dL_dimage.shape and background.device == dL_dimage.device,
                 f"background must have dL_dimage's shape {tuple(dL_dimage.shape)} and device")
    dev = dL_dimage.device
    v = _image_view(h, w)
    g, t, b = dL_dimage.contiguous(), final_T.contiguous(), background.contiguous()
    d_alpha = torch.empty((h, w), dtype=torch.float32, device=dev)
    d_bg = torch.empty_like(g) if want_background_grad else None
    check(lib.cugs_envmap_composite_backward(C.byref(v), None, _ptr(b), _ptr(g), _ptr(t), 1.0, None, 0, _ptr(d_alpha),
                                             None, _ptr(d_bg), None, _stream(dev)), "cugs_envmap_composite_backward")
    return d_alpha, d_bg


def render_with_environment(model: GaussianModel, camera: CameraInfo, settings: RenderSettings, env: EnvironmentMap,
                            **render_kwargs) -> Tuple[torch.Tensor, RenderOutput]:
    """(image, render_out): render(model, camera, settings, **render_kwargs) on background 0 and the composite behind it.
    render_out.color stays the background-free C; give render_out to composite_environment_backward and
    render_backward."""
    _require_zero_background(settings, "render_with_environment")
    out = render(model, camera, settings, **render_kwargs)
    return composite_environment(out, camera, env), out
