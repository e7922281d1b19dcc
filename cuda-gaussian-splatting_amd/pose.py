"""Camera pose helpers over render_backward(..., want_camera_grad=True) (not in the reference).

The camera gradient comes back as dL/d(view), view = CameraInfo.world_to_camera() (4x4, row 3 zero).  A pose
optimizer works in a minimal parameterisation instead: a left-multiplied perturbation view' = Exp(xi) view with
xi = (rho, phi) in se(3) - rho a translation, phi a rotation vector, both in the camera frame.

    g = viewmat_grad_to_se3(out.dL_dviewmat, camera)     # dL/dxi at xi = 0, a [6] device tensor
    camera = apply_se3(camera, -lr * g)                   # one gradient step on the pose
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from .types import CameraInfo


def _hat(phi: torch.Tensor) -> torch.Tensor:
    z = torch.zeros((), dtype=phi.dtype, device=phi.device)
    return torch.stack([torch.stack([z, -phi[2], phi[1]]), torch.stack([phi[2], z, -phi[0]]),
                        torch.stack([-phi[1], phi[0], z])])


def se3_exp(xi: torch.Tensor) -> torch.Tensor:
    """The 4x4 matrix Exp(xi) of xi = (rho, phi) (Rodrigues' formula and the left Jacobian V, series near 0); in the
    dtype and on the device of xi, differentiable."""
    rho, phi = xi[:3], xi[3:]
    theta2 = (phi * phi).sum()
    K = _hat(phi)
    K2 = K @ K
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    small = bool(theta2 < 1e-12)
    if small:       # Taylor terms: sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3
        a, b, c = 1.0 - theta2 / 6.0, 0.5 - theta2 / 24.0, 1.0 / 6.0 - theta2 / 120.0
    else:
        theta = torch.sqrt(theta2)
        a, b, c = torch.sin(theta) / theta, (1.0 - torch.cos(theta)) / theta2, (theta - torch.sin(theta)) / (theta2 * theta)
    R = eye + a * K + b * K2
    V = eye + b * K + c * K2
    top = torch.cat([R, (V @ rho).reshape(3, 1)], dim=1)
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=xi.dtype, device=xi.device)
    return torch.cat([top, bottom], dim=0)


def viewmat_grad_to_se3(dL_dviewmat: torch.Tensor, camera: CameraInfo) -> torch.Tensor:
    """dL/dxi of view' = Exp(xi) view at xi = 0: [dL/drho, dL/dphi] = [G_t, (A21 - A12, A02 - A20, A10 - A01)] with
    A = G_R R^T + G_t t^T, G_R the upper-left 3x3 block of dL_dviewmat and G_t its fourth column.  A [6] tensor on the
    device and in the dtype of dL_dviewmat; no host sync."""
    if tuple(dL_dviewmat.shape) != (4, 4):
        raise ValueError("dL_dviewmat must be [4, 4]")
    view = torch.as_tensor(camera.world_to_camera(), dtype=dL_dviewmat.dtype).to(dL_dviewmat.device, non_blocking=True)
    G_R, G_t = dL_dviewmat[:3, :3], dL_dviewmat[:3, 3]
    A = G_R @ view[:3, :3].T + torch.outer(G_t, view[:3, 3])
    return torch.cat([G_t, torch.stack([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]])])


def apply_se3(camera: CameraInfo, xi) -> CameraInfo:
    """The camera with view' = Exp(xi) view: composed in float64, stored as float32 (CameraInfo's precision).  xi: six
    numbers (tensor, array or sequence), (rho, phi)."""
    x = torch.as_tensor(np.asarray(torch.as_tensor(xi).detach().cpu(), dtype=np.float64), dtype=torch.float64)
    if x.shape != (6,) or not bool(torch.isfinite(x).all()):
        raise ValueError("xi must be six finite numbers")
    view = torch.as_tensor(camera.world_to_camera(), dtype=torch.float64)
    out = (se3_exp(x) @ view).numpy()
    return dataclasses.replace(camera, rotation=out[:3, :3].astype(np.float32),
                               translation=out[:3, 3].astype(np.float32).copy())


def rotation_angle_deg(R_a: np.ndarray, R_b: np.ndarray) -> float:
    """Angle of R_a R_b^T in degrees (pose error of two camera rotations)."""
    M = np.asarray(R_a, dtype=np.float64) @ np.asarray(R_b, dtype=np.float64).T
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(M) - 1.0) / 2.0))))
