"""CPU mirror of the exposure-compensated, masked loss (csrc/loss.hip EXPO kernels, cugs_amd.combined_loss_exposure;
DESIGN.md 4.18): the reference's own loss ops (oracle/loss_oracle.py) on

    x' = m (c A^T + b)       y' = m y

built with torch ops, and autograd for dL/dc and dL/dE.  Nothing in the reference does this, so this is the yardstick;
tests/test_exposure_ref.py checks it against the same ops in float64.  AdamMirror is torch.optim.Adam on one row,
for ExposureModel.step.  Shared by the CPU and GPU tests; cases are computed once, callers must not modify them."""
import numpy as np
import torch

from metrics_ref import loss_oracle

# (h, w): less than one tile | 2 x 3 partial tiles, halos crossing tile and image edges | ragged, both radius routes |
# full tiles only
SHAPES = [(7, 5), (17, 33), (37, 53), (64, 64)]


def make_case(h, w):
    """(c, t, E, mask) float32 CPU tensors, seeded by the shape.  The mask has zeros and fractional weights."""
    g = torch.Generator().manual_seed(h * 1000 + w)
    t = torch.rand((h, w, 3), generator=g)
    c = (t + 0.2 * torch.randn((h, w, 3), generator=g)).clamp(0, 1.5)
    E = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1) + 0.1 * torch.randn((3, 4), generator=g)
    mask = (torch.rand((h, w), generator=g) > 0.3).float() * torch.rand((h, w), generator=g).clamp(0.25, 1.0)
    return c, t, E.contiguous(), mask.contiguous()


def correct(c, E, mask=None):
    """x' = m (c A^T + b) with E = [A | b]."""
    x = c @ E[:, :3].T + E[:, 3]
    return x if mask is None else x * mask.unsqueeze(-1)


def mirror(c, t, E=None, mask=None, lambda_=0.2, window_size=11, dtype=torch.float32):
    """dict(loss, l1, ssim_mean as floats; dL_dcolor [H,W,3], dL_dexposure [3,4] (None without E), corrected [H,W,3]
    as numpy arrays of `dtype`)."""
    lo = loss_oracle()
    c = c.to(dtype).clone().requires_grad_(True)
    t = t.to(dtype)
    Ev = None if E is None else E.to(dtype).clone().requires_grad_(True)
    m = None if mask is None else mask.to(dtype)
    x = correct(c, Ev, m) if Ev is not None else (c if m is None else c * m.unsqueeze(-1))
    y = t if m is None else t * m.unsqueeze(-1)
    kernel = lo.gaussian_kernel(window_size).to(dtype)
    if dtype == torch.float32:
        l1, ss = lo.l1_loss(x, y), lo.ssim(x, y, window_size).mean()
    else:                                   # the same ops with the window in `dtype` (gaussian_kernel is float32)
        l1, ss = (x - y).abs().mean(), _ssim_mean(x, y, kernel, window_size)
    loss = (1.0 - lambda_) * l1 + lambda_ * (1.0 - ss)
    loss.backward()
    return dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim_mean=float(ss.detach()), dL_dcolor=c.grad.numpy().copy(),
                dL_dexposure=None if Ev is None else Ev.grad.numpy().copy(), corrected=x.detach().numpy().copy())


def _ssim_mean(x, y, kernel, window_size):
    """loss_oracle.ssim's op sequence with a caller-supplied window (for the float64 run)."""
    import torch.nn.functional as F
    pad = window_size // 2
    xp, yp = x.permute(2, 0, 1).unsqueeze(0), y.permute(2, 0, 1).unsqueeze(0)
    conv = lambda a: F.conv2d(a, kernel, None, 1, pad, 1, 3)
    mu_x, mu_y = conv(xp), conv(yp)
    sx, sy, sxy = conv(xp * xp) - mu_x * mu_x, conv(yp * yp) - mu_y * mu_y, conv(xp * yp) - mu_x * mu_y
    c1, c2 = 0.01 * 0.01, 0.03 * 0.03
    smap = ((2.0 * mu_x * mu_y + c1) * (2.0 * sxy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (sx + sy + c2))
    return smap.squeeze(0).permute(1, 2, 0).mean(dim=2).mean()


_cache = {}


def case(h, w, masked, lambda_=0.2, window_size=11):
    """(c, t, E, mask or None, mirror dict) of a shape, computed once and shared."""
    key = (h, w, masked, lambda_, window_size)
    if key not in _cache:
        c, t, E, mask = make_case(h, w)
        mask = mask if masked else None
        _cache[key] = (c, t, E, mask, mirror(c, t, E, mask, lambda_, window_size))
    return _cache[key]


class AdamMirror:
    """torch.optim.Adam on one [3,4] row, for ExposureModel.step: step(grad, lr) returns the row after the update."""

    def __init__(self, row0, beta1=0.9, beta2=0.999, eps=1e-15):
        self.p = row0.clone().to(torch.float32).reshape(3, 4).requires_grad_(True)
        self.opt = torch.optim.Adam([self.p], lr=1.0, betas=(beta1, beta2), eps=eps)

    def step(self, grad, lr):
        self.opt.param_groups[0]["lr"] = float(lr)
        self.p.grad = torch.as_tensor(grad, dtype=torch.float32).reshape(3, 4).clone()
        self.opt.step()
        return self.p.detach().clone()


def identity():
    return torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).contiguous()
