"""fp64 torch-autograd model of the whole projection stage: pose_ref.project (the camera-space point, J, Sigma', the
conic, the 2-D mean, z) with the opacity's sigmoid and the SH colour added, so that ONE vector-Jacobian product gives
all five parameter gradients of project_backward.

Written from the equations, sharing no code with oracle/cugs_oracle.c or the kernels:
  opacity_act = sigmoid(opacity)
  rgb_c = relu(sum_k sh[c, k] Y_k(d) + 0.5),  d = (p - C) / max(|p - C|, 1e-8),  C = -W^T tvec, d DETACHED (the reference
          holds the view direction constant in its backward); Y is test_oracle_autograd._sh_basis; only the
          first (degree + 1)^2 coefficients are active
  L = <g_means, means_2d> + <g_conic, (a, b, c)> + <g_rgb, rgb> + <g_opa, opacity_act> [+ <g_z, z>]
with the conic's off-diagonal in the stored-b convention of pose_ref (b = (inv01 + inv10) / 2).  Culling is piecewise
constant in the parameters and is taken from the caller (`live`, e.g. radii > 0): a culled row's gradients are zero.
"""
import numpy as np
import torch

import pose_ref
from pose_ref import D, _t
from test_oracle_autograd import _sh_basis

NAMES = ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs")
SH_C0 = 0.28209479177387814


def render_backward(arrays, cam, fwd, bg, g, g_depth=None, g_alpha=None):
    """The fp64 render model of tests/test_oracle_autograd.py (_render_autograd, imported, not copied) on the Gaussians
    the forward kept: (maps, grads) with maps = {color [h,w,3], and with their gradients given depth_map, alpha [h,w]} and
    grads the five parameter gradients (float64 numpy, full size, culled rows zero) of
    <g, color> + <g_depth, depth_map> + <g_alpha, alpha>.

    `fwd` is the oracle's forward: its tile lists and depth order are piecewise constant in the parameters.  The depth
    map sum_i z_i alpha_i T_i and alpha = 1 - T_final are the SAME blend with another colour - (z_i, 0, 0), z = t.z a
    function of the positions, over a black background, and (1, 1, 1) - so they go through _render_autograd too, with
    SH coefficients that produce those colours (degree-0 coefficient (colour - 0.5) / Y_0, the rest zero)."""
    from test_oracle_autograd import _render_autograd
    w, h = cam.width, cam.height
    live = np.flatnonzero(fwd["radii"] > 0)
    n, m = fwd["radii"].shape[0], live.size
    slot = np.full(n, -1)
    slot[live] = np.arange(m)
    ntx = (w + 15) // 16
    member = np.zeros((h * w, m), bool)
    tr, vals = fwd["tile_ranges"], fwd["values"]
    for py in range(h):
        for px in range(w):
            s, e = tr[(py // 16) * ntx + px // 16]
            member[py * w + px, slot[vals[s:e]]] = True
    order = np.argsort(fwd["depths"][live], kind="stable")
    p = {k: torch.tensor(v[live], dtype=D, requires_grad=True) for k, v in arrays.items()}
    color = _render_autograd(p, cam, member, order, bg)
    L = (color * _t(g)).sum()
    maps = dict(color=color.detach().numpy())
    if g_depth is not None or g_alpha is not None:
        z = (p["positions"] @ _t(cam.rotation).T + _t(cam.translation))[:, 2]
        black = (0.0, 0.0, 0.0)
        coeffs = lambda c0: torch.cat([c0.reshape(m, 1, 1).expand(m, 3, 1), torch.zeros((m, 3, 15), dtype=D)], 2)
        if g_depth is not None:
            q = dict(p, sh_coeffs=coeffs((z - 0.5) / SH_C0))
            depth = _render_autograd(q, cam, member, order, black)[:, :, 0]
            maps["depth_map"] = depth.detach().numpy()
            L = L + (depth * _t(g_depth)).sum()
        if g_alpha is not None:
            q = dict(p, sh_coeffs=coeffs(torch.full((m,), 0.5 / SH_C0, dtype=D)))
            alpha = _render_autograd(q, cam, member, order, black)[:, :, 0]
            maps["alpha"] = alpha.detach().numpy()
            L = L + (alpha * _t(g_alpha)).sum()
    L.backward()
    grads = {}
    for k, t in p.items():
        full = np.zeros(arrays[k].shape, np.float64)
        full[live] = t.grad.numpy()
        grads["dL_d" + k] = full
    return maps, grads


def _camera(cam, n):
    K = cam.intrinsics
    view = _t(cam.world_to_camera().astype(np.float32))
    f32 = lambda v: float(np.float32(v))                              # the intrinsics as the C ABI receives them
    return view[:3, :3].expand(n, 3, 3), view[:3, 3].expand(n, 3), (f32(K.fx), f32(K.fy), f32(K.cx), f32(K.cy))


def _colour(positions, sh, W, tvec, degree):
    """Raw colour sum_k c_k Y_k + 0.5 [n, 3] and its per-term magnitude sum [n, 3]; the direction is detached."""
    centre = -(W[0].T @ tvec[0])
    d = (positions - centre).detach()
    d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-8)
    active = (degree + 1) ** 2
    Y = _sh_basis(d)[:, None, :active]
    terms = sh[:, :, :active] * Y
    return terms.sum(2) + 0.5, terms.abs().sum(2) + 0.5


def forward(arrays, cam, degree=3, scale_mod=1.0):
    """fp64 numpy: means_2d [n,2], depths [n], cov_2d_inv [n,3], opacities_act [n], rgb [n,3] and rgb_mag [n,3] (the sum
    of the magnitudes of the colour's terms, which bounds an fp32 evaluation's rounding), for EVERY row - the caller
    applies the culling (t.z <= 0.2, det <= 0, radius 0)."""
    n = arrays["positions"].shape[0]
    W, tvec, (fx, fy, cx, cy) = _camera(cam, n)
    with torch.no_grad():
        means, conic, z = pose_ref.project(_t(arrays["positions"]), _t(arrays["rotations"]), _t(arrays["scales"]), W,
                                           tvec, fx, fy, cx, cy, scale_mod)
        raw, mag = _colour(_t(arrays["positions"]), _t(arrays["sh_coeffs"]), W, tvec, degree)
        return dict(means_2d=means.numpy(), depths=z.numpy(), cov_2d_inv=conic.numpy(),
                    opacities_act=torch.sigmoid(_t(arrays["opacities"])[:, 0]).numpy(),
                    rgb=raw.clamp_min(0.0).numpy(), rgb_mag=mag.numpy())


def backward(arrays, cam, g_means, g_conic, g_rgb, g_opa, g_z=None, live=None, degree=3, scale_mod=1.0):
    """dict of the five gradients (float64 numpy, the parameters' shapes) of L above.  Rows where `live` is False are
    zero in the four geometry gradients; dL_dsh_coeffs knows no culling (sh_backward runs on every row: a culled
    Gaussian's dL_drgb is zero in a real backward, and that is what keeps its row zero)."""
    n = arrays["positions"].shape[0]
    W, tvec, (fx, fy, cx, cy) = _camera(cam, n)
    p = {k: _t(arrays[k]).requires_grad_(True) for k in ("positions", "rotations", "scales", "opacities", "sh_coeffs")}
    means, conic, z = pose_ref.project(p["positions"], p["rotations"], p["scales"], W, tvec, fx, fy, cx, cy, scale_mod)
    raw, _ = _colour(p["positions"], p["sh_coeffs"], W, tvec, degree)
    rgb = torch.where(raw > 0, raw, torch.zeros_like(raw))
    opa = torch.sigmoid(p["opacities"][:, 0])
    L = ((means * _t(g_means)).sum() + (conic * _t(g_conic)).sum() + (rgb * _t(g_rgb)).sum() +
         (opa * _t(np.asarray(g_opa).reshape(n))).sum())
    if g_z is not None:
        L = L + (z * _t(np.asarray(g_z).reshape(n))).sum()
    L.backward()
    keep = np.ones(n, bool) if live is None else np.asarray(live, bool)
    out = {}
    for k, t in p.items():
        g = t.grad.numpy().copy()
        if k != "sh_coeffs":
            g[~keep] = 0.0
        out["dL_d" + k] = g
    return out
