"""References for the bilateral-grid kernels (include/cugs_hip.h; test infrastructure).

mirror_*: numpy in the header's fp32 operation order, op for op (the library builds with -ffp-contract=off), so
`corrected` and `dL_drendered` must come out with the GPU's bytes.  The grid gradient is a long sum whose order is the
kernel's own business: the mirror accumulates it in fp64 and the tests compare it by tolerance.
torch_reference: libtorch fp64 grid_sample(bilinear, align_corners=True, padding_mode="border") + einsum + autograd on
the CPU - the sequence the kernels replace, and the yardstick of both.

Shapes are (h, w, (GX, GY, L)): BilateralGridModel's grid_shape order; the grid tensor is [12, L, GY, GX]."""
from __future__ import annotations

import functools

import numpy as np

F = np.float32
LW = (F(0.299), F(0.587), F(0.114))

SHAPES = [(7, 5, (4, 3, 2)), (1, 9, (2, 2, 3)), (37, 53, (16, 16, 8)), (24, 40, (5, 3, 4)), (270, 480, (4, 4, 2))]
CLAMP_SHAPE = (24, 40, (5, 3, 4))                  # run a second time with a block of colours outside [0, 1]
CASES = [(h, w, s, False) for h, w, s in SHAPES] + [CLAMP_SHAPE + (True,)]


def case_id(c) -> str:
    h, w, (gx, gy, l), clamp = c
    return f"{h}x{w}-{gx}x{gy}x{l}" + ("-clamp" if clamp else "")


def identity_grid(grid_shape) -> np.ndarray:
    gx, gy, l = grid_shape
    eye = np.concatenate([np.eye(3, dtype=F), np.zeros((3, 1), F)], axis=1).reshape(12, 1, 1, 1)
    return np.ascontiguousarray(np.broadcast_to(eye, (12, l, gy, gx)))


@functools.lru_cache(maxsize=None)
def case(h: int, w: int, grid_shape, clamp: bool = False):
    """(grid [12,L,GY,GX], rendered [h,w,3], dL_dcorrected [h,w,3]), float32, seeded by the shape.  grid = identity + 0.3
    normal.  Colours in [0.1, 0.9], moved along (1, 1, 1) so that the fractional part of luma (L-1) lies in
    [0.05, 0.95]: the luma weights sum to 1, so the shift of the colour is the shift of the luma, and the derivative along
    z is nowhere at a kink (the rounding to float32 moves luma by 1e-7, far inside the margin).  `clamp`: a block of
    pixels gets colours above 1 and below 0 - the clamp of fz and the zero guidance gradient.  Treat the arrays as
    read-only: they are shared between the tests."""
    gx, gy, l = grid_shape
    rng = np.random.default_rng([h, w, gx, gy, l, int(clamp)])
    grid = (identity_grid(grid_shape) + 0.3 * rng.standard_normal((12, l, gy, gx))).astype(F)
    c = rng.uniform(0.1, 0.9, (h, w, 3))
    zs = (c @ np.array([0.299, 0.587, 0.114])) * (l - 1)
    frac = zs - np.floor(zs)
    c = c + ((np.clip(frac, 0.05, 0.95) - frac) / (l - 1))[..., None]
    if clamp:
        ys, xs = slice(h // 4, max(h // 2, h // 4 + 1)), slice(w // 4, max(w // 2, w // 4 + 1))
        block = c[ys, xs]
        u = rng.uniform(0.0, 0.3, block.shape[:2] + (1,))
        over = (np.add.outer(np.arange(block.shape[0]), np.arange(block.shape[1])) % 2 == 0)[..., None]
        c[ys, xs] = np.where(over, 1.2 + u, -0.1 - u)
    g = rng.standard_normal((h, w, 3))
    out = tuple(np.ascontiguousarray(a, dtype=F) for a in (grid, c, g))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the fp32 mirror ---------------------------------------------------------------------------------------------

def _coords(c: np.ndarray, dims):
    l, gy, gx = dims
    h, w = c.shape[:2]
    sx = F(gx - 1) / F(w - 1) if w > 1 else F(0)
    sy = F(gy - 1) / F(h - 1) if h > 1 else F(0)
    fx = np.arange(w, dtype=F) * sx
    fy = np.arange(h, dtype=F) * sy
    x0 = np.minimum(fx.astype(np.int32), gx - 2)
    y0 = np.minimum(fy.astype(np.int32), gy - 2)
    tx, ty = fx - x0.astype(F), fy - y0.astype(F)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    luma = (LW[0] * r + LW[1] * g) + LW[2] * b
    top = F(l - 1)
    zs = luma * top
    fz = np.minimum(np.maximum(zs, F(0)), top)
    inside = (zs >= 0) & (zs <= top)
    z0 = np.minimum(fz.astype(np.int32), l - 2)
    tz = fz - z0.astype(F)
    return (x0[None, :], y0[:, None], z0), (tx[None, :], ty[:, None], tz), inside


def _lerp(a, b, t):
    return a + t * (b - a)


def _sample(grid: np.ndarray, idx, t):
    """E, D [12,h,w]: the sliced transform and its derivative along fz."""
    (x0, y0, z0), (tx, ty, tz) = idx, t
    E, D = [], []
    for k in range(12):
        G = grid[k]
        p = []
        for z in (z0, z0 + 1):
            p.append(_lerp(_lerp(G[z, y0, x0], G[z, y0, x0 + 1], tx), _lerp(G[z, y0 + 1, x0], G[z, y0 + 1, x0 + 1], tx), ty))
        d = p[1] - p[0]
        D.append(d)
        E.append(p[0] + tz * d)
    return E, D


def mirror_slice(grid: np.ndarray, c: np.ndarray) -> np.ndarray:
    idx, t, _ = _coords(c, grid.shape[1:])
    E, _ = _sample(grid, idx, t)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    out = np.stack([((E[4 * i] * r + E[4 * i + 1] * g) + E[4 * i + 2] * b) + E[4 * i + 3] for i in range(3)], axis=-1)
    assert out.dtype == F
    return out


def mirror_backward(grid: np.ndarray, c: np.ndarray, gc: np.ndarray):
    """(dL_drendered float32 [h,w,3] in the header's order, dL_dgrid float64 [12,L,GY,GX] with fp64 sums)."""
    dims = grid.shape[1:]
    l, gy, gx = dims
    idx, t, inside = _coords(c, dims)
    E, D = _sample(grid, idx, t)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    g0, g1, g2 = gc[..., 0], gc[..., 1], gc[..., 2]
    q = [((D[4 * i] * r + D[4 * i + 1] * g) + D[4 * i + 2] * b) + D[4 * i + 3] for i in range(3)]
    s = np.where(inside, ((g0 * q[0] + g1 * q[1]) + g2 * q[2]) * F(l - 1), F(0)).astype(F)
    d_img = np.stack([((E[j] * g0 + E[4 + j] * g1) + E[8 + j] * g2) + s * LW[j] for j in range(3)], axis=-1)
    assert d_img.dtype == F

    (x0, y0, z0), (tx, ty, tz) = idx, tuple(a.astype(np.float64) for a in t)
    shape = z0.shape
    x0, y0 = np.broadcast_to(x0, shape), np.broadcast_to(y0, shape)
    prod = [gi.astype(np.float64) * cj for gi in (g0, g1, g2) for cj in (r.astype(np.float64), g.astype(np.float64),
                                                                        b.astype(np.float64), 1.0)]
    d_grid = np.zeros((12, l * gy * gx), np.float64)
    for dz, wz in ((0, 1.0 - tz), (1, tz)):
        for dy, wy in ((0, 1.0 - ty), (1, ty)):
            for dx, wx in ((0, 1.0 - tx), (1, tx)):
                flat = (((z0 + dz) * gy + (y0 + dy)) * gx + (x0 + dx)).ravel()
                wgt = np.broadcast_to(wy * wx * wz, shape)
                for k in range(12):
                    d_grid[k] += np.bincount(flat, weights=(wgt * prod[k]).ravel(), minlength=l * gy * gx)
    return d_img, d_grid.reshape(12, l, gy, gx)


def mirror_tv(grid: np.ndarray, weight: float = 1.0):
    """(tv float32, weight * dtv/dgrid float32): differences, squares and sums in fp64, as the kernel."""
    G = grid.astype(np.float64)
    tv, grad = 0.0, np.zeros_like(G)
    for axis in (1, 2, 3):
        d = np.diff(G, axis=axis)
        tv += float(np.sum(d * d)) / d.size
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        grad[tuple(hi)] += 2.0 / d.size * d
        grad[tuple(lo)] -= 2.0 / d.size * d
    return F(tv), (weight * grad).astype(F)


# ---- libtorch fp64 -----------------------------------------------------------------------------------------------

def torch_slice(grid, c):
    """The libtorch sequence on tensors of any dtype / device: grid [12,L,GY,GX], c [h,w,3] -> corrected [h,w,3]."""
    import torch
    import torch.nn.functional as nnf
    h, w = c.shape[:2]
    xs = torch.arange(w, dtype=c.dtype, device=c.device) / max(w - 1, 1)
    ys = torch.arange(h, dtype=c.dtype, device=c.device) / max(h - 1, 1)
    luma = c @ torch.tensor([0.299, 0.587, 0.114], dtype=c.dtype, device=c.device)
    at = torch.stack([xs[None, :].expand(h, w), ys[:, None].expand(h, w), luma], dim=-1) * 2 - 1
    coef = nnf.grid_sample(grid[None], at[None, None], mode="bilinear", padding_mode="border", align_corners=True)
    coef = coef[0, :, 0].reshape(3, 4, h, w)
    return torch.einsum("ijhw,hwj->hwi", coef[:, :3], c) + coef[:, 3].permute(1, 2, 0)


def torch_tv(grid):
    return sum(((grid.narrow(a, 1, grid.shape[a] - 1) - grid.narrow(a, 0, grid.shape[a] - 1)) ** 2).mean() for a in (1, 2, 3))


@functools.lru_cache(maxsize=None)
def torch_reference(h: int, w: int, grid_shape, clamp: bool = False):
    """fp64 on the CPU for case(...): dict of float64 arrays corrected, dL_drendered, dL_dgrid, tv (0-dim), dtv_dgrid."""
    import torch
    grid, c, g = (torch.from_numpy(a.astype(np.float64)) for a in case(h, w, grid_shape, clamp))
    grid.requires_grad_(True)
    c.requires_grad_(True)
    out = torch_slice(grid, c)
    d_grid, d_c = torch.autograd.grad(out, (grid, c), g)
    tv = torch_tv(grid)
    (d_tv,) = torch.autograd.grad(tv, grid)
    ref = {"corrected": out.detach().numpy(), "dL_drendered": d_c.numpy(), "dL_dgrid": d_grid.numpy(),
           "tv": tv.detach().numpy(), "dtv_dgrid": d_tv.numpy()}
    for a in ref.values():
        a.setflags(write=False)
    return ref


def err_of_scale(got, ref) -> float:
    """max |got - ref| / max |ref|: the element-wise error in units of the tensor's largest magnitude."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / max(float(np.max(np.abs(ref))), 1e-300))
