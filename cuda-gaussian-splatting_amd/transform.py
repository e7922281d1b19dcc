"""A model moved by a similarity x' = s R x + t (not in the reference).

  Similarity                 scale, rotation, translation in fp64 numpy, with inverse / compose / matrix / apply_points
  sh_rotation_matrices       the per-band SH rotation matrices D_1..D_3 of a rotation, from the C library
  transform_gaussians        the model's tensors transformed IN PLACE by one kernel launch, for all rows or a row mask
  transform_camera(s)        the camera that sees the transformed model as the old camera saw the old model
  similarity_from_cameras    the normalisation trainers apply before training: centre, radius, up axis
  merge_gaussians            the rows of a second model appended to a model (and to its FusedAdam)

On a Gaussian: positions' = s R p + t, scales' = scales + log s, rotations' = q_R (x) q (Hamilton, wxyz, q left raw),
opacities unchanged, every SH band l >= 1 of every channel multiplied by D_l(R).  A camera (Rc, tc) moves to
Rc' = Rc R^T, tc' = s tc - Rc R^T t: camera-space coordinates scale by s, so the image and alpha are unchanged and the
depth map scales by s.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .rasterizer import _ptr, _stream, _torch_check
from .types import CameraInfo, GaussianModel

_PARAMS = ("positions", "sh_coeffs", "opacities", "rotations", "scales")


def _init_abi(rotation, translation, scale) -> "_lib.Similarity":
    """cugs_similarity_init on fp64 values; a rejected transform is a ValueError."""
    R = np.ascontiguousarray(np.asarray(rotation, dtype=np.float64).reshape(9))
    t = np.ascontiguousarray(np.asarray(translation, dtype=np.float64).reshape(3))
    out = _lib.Similarity()
    dp = C.POINTER(C.c_double)
    code = lib.cugs_similarity_init(C.byref(out), R.ctypes.data_as(dp), t.ctypes.data_as(dp), float(scale))
    if code != 0:
        raise ValueError("Similarity: the rotation must be a proper rotation (within 1e-4 of orthogonal, det > 0), the "
                         "scale positive and every value finite")
    return out


@dataclasses.dataclass
class Similarity:
    """x' = scale * rotation @ x + translation; fp64 numpy values."""
    scale: float = 1.0
    rotation: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(3))
    translation: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(3))

    def __post_init__(self):
        self.scale = float(self.scale)
        self.rotation = np.array(self.rotation, dtype=np.float64).reshape(3, 3)
        self.translation = np.array(self.translation, dtype=np.float64).reshape(3)

    def matrix(self) -> np.ndarray:
        """The 4x4 matrix [[s R, t], [0, 1]]."""
        m = np.eye(4)
        m[:3, :3] = self.scale * self.rotation
        m[:3, 3] = self.translation
        return m

    @staticmethod
    def from_matrix(m) -> "Similarity":
        """The similarity of a 4x4 matrix [[s R, t], [0, 1]]: s = cbrt(det(s R))."""
        m = np.asarray(m, dtype=np.float64)
        if m.shape != (4, 4):
            raise ValueError("Similarity.from_matrix: a 4x4 matrix is needed")
        det = float(np.linalg.det(m[:3, :3]))
        if not det > 0.0:
            raise ValueError("Similarity.from_matrix: the linear part must have a positive determinant")
        s = det ** (1.0 / 3.0)
        return Similarity(s, m[:3, :3] / s, m[:3, 3])

    def inverse(self) -> "Similarity":
        Rt = self.rotation.T
        return Similarity(1.0 / self.scale, Rt, -(Rt @ self.translation) / self.scale)

    def compose(self, other: "Similarity") -> "Similarity":
        """self after other: x -> self(other(x))."""
        return Similarity(self.scale * other.scale, self.rotation @ other.rotation,
                          self.scale * (self.rotation @ other.translation) + self.translation)

    def apply_points(self, x) -> np.ndarray:
        """[..., 3] points, fp64."""
        x = np.asarray(x, dtype=np.float64)
        return self.scale * (x @ self.rotation.T) + self.translation

    def is_pure_translation(self) -> bool:
        return self.scale == 1.0 and bool(np.array_equal(self.rotation, np.eye(3)))

    def to_abi(self) -> "_lib.Similarity":
        """The filled CugsSimilarity: what the kernel multiplies by, fp32 rounded once from fp64."""
        return _init_abi(self.rotation, self.translation, self.scale)


def sh_rotation_matrices(rotation) -> List[np.ndarray]:
    """[D1 (3x3), D2 (5x5), D3 (7x7)] float32 of a rotation matrix, in the basis and sign convention the projection
    evaluates: Y_l(R d) = D_l Y_l(d), so coefficients move by c' = D_l c.  For per-Gaussian SH-like features kept
    outside the model."""
    s = _init_abi(rotation, np.zeros(3), 1.0)
    return [np.array(s.d1, dtype=np.float32).reshape(3, 3), np.array(s.d2, dtype=np.float32).reshape(5, 5),
            np.array(s.d3, dtype=np.float32).reshape(7, 7)]


def transform_gaussians(model: GaussianModel, sim: Similarity, mask: Optional[torch.Tensor] = None,
                        optimizer=None) -> None:
    """Moves `model` by `sim` IN PLACE: one launch of cugs_transform_gaussians on the current stream, no host sync, no
    temporaries.  `mask` (bool [N] on the model's device): only the rows set are moved; the others are neither read nor
    written and keep every bit.  The tensors must be contiguous float32 (views at any dword offset are fine).
    `optimizer` (the FusedAdam built on `model`): a pure translation leaves its moments alone - every gradient is
    invariant under it.  Otherwise the moments m_ / v_ of the transformed rows of the positions, rotations and SH groups
    are set to zero in the same launch (element-wise second moments are not covariant under a rotation), as the new
    rows of a densification and the late-seen rows of sparse Adam start from zero moments; the scales and opacities
    groups keep theirs (their gradients are invariant) and step_count_ is unchanged.
    Per-Gaussian state held elsewhere is the caller's, as for prune_gaussians: DensificationController accumulators, an
    MCMCController, parallel.py's replicas."""
    _torch_check(model.is_valid(), "GaussianModel is not valid")
    _torch_check(model.positions.is_cuda, "GaussianModel must be on CUDA device")
    n = model.num_gaussians()
    dev = model.positions.device
    coeffs = int(model.sh_coeffs.shape[2])
    _torch_check(coeffs in (1, 4, 9, 16), f"transform_gaussians: sh_coeffs has {coeffs} coefficients, not 1, 4, 9 or 16")
    for name in ("positions", "rotations", "scales", "sh_coeffs"):
        t = getattr(model, name)
        _torch_check(t.dtype == torch.float32 and t.is_contiguous(),
                     f"transform_gaussians: {name} must be contiguous float32 (the update is in place)")
    if mask is not None:
        _torch_check(isinstance(mask, torch.Tensor) and mask.dtype == torch.bool and mask.dim() == 1 and
                     int(mask.shape[0]) == n, f"transform_gaussians: mask must be a bool tensor of shape [{n}]")
        _torch_check(mask.device == dev, "transform_gaussians: mask must be on the model's device")
        mask = mask.contiguous().view(torch.uint8)
    xf = sim.to_abi()
    zero: List[torch.Tensor] = []
    if optimizer is not None and not sim.is_pure_translation():
        _torch_check(optimizer.model_ is model, "transform_gaussians: the optimizer was built on another model")
        for g in (0, 1, 4):                                     # ParamGroup kPositions, kSHCoeffs, kRotations
            for t in (optimizer.m_[g], optimizer.v_[g]):
                _torch_check(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and int(t.shape[0]) == n,
                             "transform_gaussians: the optimizer's moments must be contiguous float32 [N, ...]")
                zero.append(t)
    if n == 0:
        return
    rows = (C.c_void_p * max(len(zero), 1))(*[t.data_ptr() for t in zero])
    floats = (C.c_int * max(len(zero), 1))(*[int(t.numel() // n) for t in zero])
    check(lib.cugs_transform_gaussians(n, coeffs, _ptr(model.positions), _ptr(model.rotations), _ptr(model.scales),
                                       _ptr(model.sh_coeffs), _ptr(mask), rows, floats, len(zero), C.byref(xf),
                                       _stream(dev)), "cugs_transform_gaussians")


def transform_camera(cam: CameraInfo, sim: Similarity) -> CameraInfo:
    """The camera that sees a model moved by `sim` as `cam` saw it before: Rc' = Rc R^T, tc' = s tc - Rc R^T t (from
    Rc' (s R x + t) + tc' = s (Rc x + tc) for every x).  Computed in fp64, stored as float32; a new CameraInfo."""
    Rc = np.asarray(cam.rotation, dtype=np.float64)
    tc = np.asarray(cam.translation, dtype=np.float64)
    Rn = Rc @ sim.rotation.T
    tn = sim.scale * tc - Rn @ sim.translation
    return dataclasses.replace(cam, intrinsics=dataclasses.replace(cam.intrinsics), rotation=Rn.astype(np.float32),
                               translation=tn.astype(np.float32))


def transform_cameras(cams: Sequence[CameraInfo], sim: Similarity) -> List[CameraInfo]:
    return [transform_camera(c, sim) for c in cams]


def _rotation_between(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The rotation of least angle that takes unit vector a to unit vector b (Rodrigues); for a = -b the half turn
    about the coordinate axis least aligned with a, made orthogonal to it."""
    v = np.cross(a, b)
    c = float(a @ b)
    if c < -1.0 + 1e-12:
        e = np.zeros(3)
        e[int(np.argmin(np.abs(a)))] = 1.0
        u = e - (e @ a) * a
        u /= np.linalg.norm(u)
        return 2.0 * np.outer(u, u) - np.eye(3)
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + K + (K @ K) / (1.0 + c)


def similarity_from_cameras(cameras: Sequence[CameraInfo], radius: float = 1.0, up=(0.0, 0.0, 1.0)) -> Similarity:
    """The scene normalisation: the similarity after which the mean camera centre is the origin, the farthest camera
    centre lies at distance `radius` and - with `up` not None - the mean camera up vector (-y of the camera axes, in
    world coordinates) points along `up`.  fp64 numpy, deterministic."""
    if len(cameras) == 0:
        raise ValueError("similarity_from_cameras: no cameras")
    Rs = [np.asarray(c.rotation, dtype=np.float64) for c in cameras]
    centres = np.stack([-(R.T @ np.asarray(c.translation, dtype=np.float64)) for R, c in zip(Rs, cameras)])
    mean = centres.mean(axis=0)
    far = float(np.max(np.linalg.norm(centres - mean, axis=1)))
    s = float(radius) / far if far > 0.0 else 1.0
    R = np.eye(3)
    if up is not None:
        ups = np.stack([-Rc[1, :] for Rc in Rs]).mean(axis=0)   # row 1 of world-to-camera: the camera's +y in the world
        nrm = float(np.linalg.norm(ups))
        target = np.asarray(up, dtype=np.float64)
        if nrm > 0.0:
            R = _rotation_between(ups / nrm, target / np.linalg.norm(target))
    return Similarity(s, R, -s * (R @ mean))


def _pad_coeffs(t: torch.Tensor, coeffs: int) -> torch.Tensor:
    """[N,3,c] zero-padded to [N,3,coeffs]."""
    if int(t.shape[2]) == coeffs:
        return t
    out = torch.zeros((t.shape[0], 3, coeffs), dtype=t.dtype, device=t.device)
    out[:, :, :t.shape[2]] = t
    return out


def merge_gaussians(model: GaussianModel, other: GaussianModel, optimizer=None) -> int:
    """Appends the rows of `other` to `model`, in order, and replaces the model's five tensors (new tensors); returns
    the new N.  Models of different SH degree meet at the higher one: the lower one's coefficients are padded with
    zeros.  With `optimizer` (the FusedAdam built on `model`) its moments follow: the old rows keep theirs bit for bit
    (zero-padded the same way), the new rows start from zero moments, pending gradients are cleared.  Tensor plumbing,
    no kernel; `other` is not modified.  State held elsewhere is the caller's, as for prune_gaussians."""
    _torch_check(model.is_valid() and other.is_valid(), "GaussianModel is not valid")
    _torch_check(other.positions.device == model.positions.device, "merge_gaussians: the models are on different devices")
    coeffs = max(int(model.sh_coeffs.shape[2]), int(other.sh_coeffs.shape[2]))
    if optimizer is not None:
        _torch_check(optimizer.model_ is model, "merge_gaussians: the optimizer was built on another model")
    n_new = other.num_gaussians()
    for name in _PARAMS:
        a, b = getattr(model, name), getattr(other, name)
        if name == "sh_coeffs":
            a, b = _pad_coeffs(a, coeffs), _pad_coeffs(b, coeffs)
        setattr(model, name, torch.cat([a, b.to(a.dtype)], dim=0).contiguous())
    if optimizer is not None:
        for g, name in enumerate(optimizer._names):
            for moments in (optimizer.m_, optimizer.v_):
                old = moments[g]
                if name == "sh_coeffs":
                    old = _pad_coeffs(old, coeffs)
                fresh = torch.zeros((n_new,) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
                moments[g] = torch.cat([old, fresh], dim=0).contiguous()
        optimizer.grads_ = [None] * optimizer.kNumGroups
    return model.num_gaussians()
