"""fp64 torch-autograd model of the projection as the camera sees it, for the camera-pose tests.

Every Gaussian gets its own leaf copy of the camera's W (3x3) and tvec, so one VJP yields each Gaussian's twelve camera
terms (dL/dW row-major, then dL/dtvec) - the rows the POSE kernel writes.  The forward follows cugs_gaussian_math.h:
t = W p + tvec; J from 1 / (t.z + 1e-6); Sigma' = (J W) Sigma (J W)^T + 0.3 I; the conic (a, b, c) = the entries
(00, 01, 11) of Sigma'^-1; means_2d = (fx t.x / t.z + cx, fy t.y / t.z + cy); z = t.z.  The off-diagonal is the
stored-b convention (Q3): L = g_a a + g_b b + g_c c with b = (inv01 + inv10) / 2, i.e. dL/dinv01 = g_b / 2, as the
kernel's grad_cov_from_inv reads it.  The SH view direction is not modelled (Q4).
"""
import numpy as np
import torch

D = torch.float64


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=D)


def rotation_matrices(q):
    q = q / torch.sqrt((q * q).sum(-1, keepdim=True) + 1e-12)
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def project(positions, rotations, scales, W, tvec, fx, fy, cx, cy, scale_mod=1.0):
    """fp64 tensors; W [n,3,3], tvec [n,3] (per-Gaussian copies).  Returns means_2d [n,2], conic [n,3], z [n]."""
    R = rotation_matrices(rotations)
    s = torch.exp(scales + float(np.log(np.float32(scale_mod) + np.float32(1e-8))))
    M = R * s.unsqueeze(-2)
    Sigma = M @ M.transpose(-1, -2)
    t = (W @ positions.unsqueeze(-1)).squeeze(-1) + tvec
    tz_inv = 1.0 / (t[:, 2] + 1e-6)
    zero = torch.zeros_like(tz_inv)
    J = torch.stack([torch.stack([fx * tz_inv, zero, -fx * t[:, 0] * tz_inv * tz_inv], -1),
                     torch.stack([zero, fy * tz_inv, -fy * t[:, 1] * tz_inv * tz_inv], -1)], -2)
    T = J @ W
    cov = T @ Sigma @ T.transpose(-1, -2) + 0.3 * torch.eye(2, dtype=D)
    inv = torch.linalg.inv(cov)
    conic = torch.stack([inv[:, 0, 0], 0.5 * (inv[:, 0, 1] + inv[:, 1, 0]), inv[:, 1, 1]], -1)
    means = torch.stack([fx * t[:, 0] / t[:, 2] + cx, fy * t[:, 1] / t[:, 2] + cy], -1)
    return means, conic, t[:, 2]


def camera_rows(arrays, cam, g_means, g_conic, g_z=None, scale_mod=1.0, live=None):
    """[n,12] float64: each Gaussian's VJP of (g_means, g_conic, g_z) with respect to its copy of (W, tvec), zero where
    `live` ([n] bool, e.g. radii > 0) is False."""
    n = arrays["positions"].shape[0]
    K = cam.intrinsics
    view = _t(cam.world_to_camera().astype(np.float32))
    W = view[:3, :3].expand(n, 3, 3).clone().requires_grad_(True)
    tv = view[:3, 3].expand(n, 3).clone().requires_grad_(True)
    means, conic, z = project(_t(arrays["positions"]), _t(arrays["rotations"]), _t(arrays["scales"]), W, tv,
                              float(K.fx), float(K.fy), float(K.cx), float(K.cy), scale_mod)
    L = (means * _t(g_means)).sum() + (conic * _t(g_conic)).sum()
    if g_z is not None:
        L = L + (z * _t(g_z)).sum()
    L.backward()
    rows = torch.cat([W.grad.reshape(n, 9), tv.grad], 1)
    if live is not None:
        rows = rows * _t(np.asarray(live, dtype=np.float64)).unsqueeze(1)
    return rows.detach().numpy()


def position_grads(arrays, cam, g_means, g_conic, scale_mod=1.0):
    """dL/dpositions of the same model (fp64), for pinning it to the oracle's project_backward."""
    n = arrays["positions"].shape[0]
    K = cam.intrinsics
    view = _t(cam.world_to_camera().astype(np.float32))
    p = _t(arrays["positions"]).requires_grad_(True)
    means, conic, _ = project(p, _t(arrays["rotations"]), _t(arrays["scales"]), view[:3, :3].expand(n, 3, 3),
                              view[:3, 3].expand(n, 3), float(K.fx), float(K.fy), float(K.cx), float(K.cy), scale_mod)
    ((means * _t(g_means)).sum() + (conic * _t(g_conic)).sum()).backward()
    return p.grad.numpy()
