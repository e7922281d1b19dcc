"""A model made smaller per Gaussian: k-means codebooks for the SH bands l >= 1, 16-bit geometry, a compact file (not
in the reference).

  vq_assign                  the nearest code of every row, by cugs_vq_assign (f32 MFMA, an exact fmaf chain)
  vq_fit                     Lloyd's k-means on the device: assign, then a deterministic fixed-point update, per iteration
  compress_gaussians         GaussianModel -> CompressedGaussians (SH rest rows replaced by a uint16 index into a codebook)
  decompress_gaussians       CompressedGaussians -> GaussianModel (fp32, the project's [N,3,C] layout)
  write_compressed / read_compressed / nbytes   an uncompressed .npz of exactly the container's arrays

The two kernels are the hot path; the gathers, casts and the decode are torch plumbing.  The arithmetic of the kernels
is stated in include/cugs_hip.h and mirrored in numpy by tests/vq_ref.py.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import check, lib
from .rasterizer import _ptr, _stream, _torch_check
from .types import GaussianModel, sh_coeff_count

VQ_MAX_DIM = 48
VQ_MAX_CODES = 65536
FORMAT_VERSION = 1
_FIELDS = ("positions", "sh_dc", "opacities", "scales", "rotations", "sh_index", "sh_codebook")


def vq_frac_bits(n: int, x_max: float, w_max: float = 1.0) -> int:
    """The fraction bits F of the fixed-point sums of cugs_vq_update for n rows with |x| <= x_max and weights
    <= w_max: with n < 2^a and max(w_max x_max, w_max) < 2^b (a, b the binary exponents frexp gives), F = 61 - a - b, so
    that every sum stays below 2^61; at most 62.  ValueError where the data leave no room (F < 0) or are not finite."""
    x_max, w_max = float(x_max), float(w_max)
    if not (math.isfinite(x_max) and math.isfinite(w_max)) or w_max < 0.0:
        raise ValueError("vq_fit: the data and the weights must be finite and the weights non-negative")
    big = max(w_max * x_max, w_max)
    if big <= 0.0:
        return 62
    bits = 61 - math.frexp(float(max(int(n), 1)))[1] - math.frexp(big)[1]
    if bits < 0:
        raise ValueError("vq_fit: n * max|w x| is too large for 64-bit fixed-point sums")
    return min(bits, 62)


def _rows(x: torch.Tensor, what: str) -> torch.Tensor:
    """[n, d] float32 on a GPU with unit element stride; a row stride >= d is passed through as ldx."""
    _torch_check(isinstance(x, torch.Tensor) and x.dim() == 2, f"{what} must be a 2-D tensor")
    _torch_check(x.is_cuda and x.dtype == torch.float32, f"{what} must be float32 on a CUDA device")
    _torch_check(1 <= int(x.shape[1]) <= VQ_MAX_DIM, f"{what}: 1 <= d <= {VQ_MAX_DIM}, got {int(x.shape[1])}")
    if x.shape[0] <= 1 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        return x.contiguous()
    return x


def _ldx(x: torch.Tensor) -> int:
    return int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1])


def _workspace(k: int, d: int, dev) -> torch.Tensor:
    size = int(lib.cugs_vq_workspace_bytes(k, d))
    _torch_check(size > 0, f"vq: no workspace for k = {k}, d = {d}")
    return torch.empty(size, dtype=torch.uint8, device=dev)


def _assign_into(x, codebook, assign, dist, ws) -> None:
    n, d, k = int(x.shape[0]), int(x.shape[1]), int(codebook.shape[0])
    with torch.cuda.device(x.device):
        check(lib.cugs_vq_assign(n, d, k, _ptr(x), _ldx(x), _ptr(codebook), _ptr(assign), _ptr(dist), _ptr(ws),
                                 ws.numel(), _stream(x.device)), "cugs_vq_assign")


def vq_assign(x: torch.Tensor, codebook: torch.Tensor, return_dist: bool = False):
    """indices int32 [n]: for every row of x [n, d] the nearest row of codebook [k, d] (the lowest index among equally
    near ones; a row holding a NaN gets 0).  With return_dist also the squared distance to it, float32 [n]."""
    x = _rows(x, "x")
    _torch_check(isinstance(codebook, torch.Tensor) and codebook.dim() == 2 and codebook.shape[1] == x.shape[1],
                 "vq_assign: codebook must be [k, d]")
    _torch_check(codebook.device == x.device and codebook.dtype == torch.float32,
                 "vq_assign: codebook must be float32 on the device of x")
    k = int(codebook.shape[0])
    _torch_check(1 <= k <= VQ_MAX_CODES, f"vq_assign: 1 <= k <= {VQ_MAX_CODES}, got {k}")
    codebook = codebook.contiguous()
    n = int(x.shape[0])
    assign = torch.empty(n, dtype=torch.int32, device=x.device)
    dist = torch.empty(n, dtype=torch.float32, device=x.device) if return_dist else None
    if n > 0:
        _assign_into(x, codebook, assign, dist, _workspace(k, int(x.shape[1]), x.device))
    return (assign, dist) if return_dist else assign


def vq_update(x: torch.Tensor, assign: torch.Tensor, codebook: torch.Tensor, frac_bits: int,
              weights: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
              workspace: Optional[torch.Tensor] = None) -> None:
    """One Lloyd update of `codebook` IN PLACE by cugs_vq_update: every code becomes the weighted fixed-point mean of
    the rows assigned to it; a code without weight keeps its bits; rows with assign = -1 are left out.  `counts`
    (int32 [k], optional) receives the member counts."""
    x = _rows(x, "x")
    n, d, k = int(x.shape[0]), int(x.shape[1]), int(codebook.shape[0])
    _torch_check(codebook.is_contiguous() and codebook.dtype == torch.float32 and tuple(codebook.shape) == (k, d) and
                 codebook.device == x.device, "vq_update: codebook must be contiguous float32 [k, d] on the device of x")
    _torch_check(assign.dtype == torch.int32 and tuple(assign.shape) == (n,) and assign.is_contiguous() and
                 assign.device == x.device, "vq_update: assign must be contiguous int32 [n]")
    if weights is not None:
        _torch_check(weights.dtype == torch.float32 and tuple(weights.shape) == (n,) and weights.is_contiguous() and
                     weights.device == x.device, "vq_update: weights must be contiguous float32 [n]")
    if counts is not None:
        _torch_check(counts.dtype == torch.int32 and tuple(counts.shape) == (k,) and counts.is_contiguous() and
                     counts.device == x.device, "vq_update: counts must be contiguous int32 [k]")
    if n == 0:
        if counts is not None:
            counts.zero_()
        return
    ws = workspace if workspace is not None else _workspace(k, d, x.device)
    with torch.cuda.device(x.device):
        check(lib.cugs_vq_update(n, d, k, _ptr(x), _ldx(x), _ptr(weights), _ptr(assign), int(frac_bits), _ptr(codebook),
                                 _ptr(counts), _ptr(ws), ws.numel(), _stream(x.device)), "cugs_vq_update")


def vq_fit(x: torch.Tensor, k: int, iters: int = 10, weights: Optional[torch.Tensor] = None,
           init: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Lloyd's k-means of the rows of x [n, d]: (codebook float32 [k', d], indices int32 [n], counts int32 [k']) with
    k' = min(k, n).  The first codebook is `init` ([k', d]) or the rows (j n) // k' of x; every iteration assigns and
    updates; a last assignment makes the indices those of the returned codebook, and counts their histogram.  Empty
    codes keep their value.  Deterministic: the same bytes from run to run.  One host read per call (the magnitudes
    the fixed-point scale derives from), none per iteration."""
    x = _rows(x, "x")
    n, d = int(x.shape[0]), int(x.shape[1])
    _torch_check(1 <= int(k) <= VQ_MAX_CODES, f"vq_fit: 1 <= k <= {VQ_MAX_CODES}, got {k}")
    _torch_check(int(iters) >= 0, "vq_fit: iters must not be negative")
    dev = x.device
    kk = min(int(k), n)
    if weights is not None:
        _torch_check(isinstance(weights, torch.Tensor) and weights.numel() == n and weights.device == dev,
                     "vq_fit: weights must hold one value per row, on the device of x")
        weights = weights.reshape(n).to(torch.float32).contiguous()
    if n == 0:
        return (torch.empty((0, d), dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev))
    if init is not None:
        _torch_check(tuple(init.shape) == (kk, d), f"vq_fit: init must be [{kk}, {d}]")
        codebook = init.to(device=dev, dtype=torch.float32).contiguous().clone()
    else:
        first = (torch.arange(kk, dtype=torch.int64, device=dev) * n) // kk
        codebook = x[first].contiguous()
    top = [x.abs().max()] + ([weights.max(), weights.min()] if weights is not None else [])
    top = torch.stack(top).tolist()                               # the one host read of a fit
    if weights is not None and not top[2] >= 0.0:
        raise ValueError("vq_fit: the weights must be non-negative")
    frac_bits = vq_frac_bits(n, top[0], top[1] if weights is not None else 1.0)
    ws = _workspace(kk, d, dev)
    assign = torch.empty(n, dtype=torch.int32, device=dev)
    for _ in range(int(iters)):
        _assign_into(x, codebook, assign, None, ws)
        vq_update(x, assign, codebook, frac_bits, weights=weights, workspace=ws)
    _assign_into(x, codebook, assign, None, ws)
    counts = torch.bincount(assign.to(torch.int64), minlength=kk).to(torch.int32)
    return codebook, assign, counts


@dataclasses.dataclass
class CompressedGaussians:
    """positions fp32 [N,3]; sh_dc [N,3], opacities [N,1], scales [N,3], rotations [N,4] in the geometry dtype;
    sh_index uint16 [N] into sh_codebook fp32 [K, 3 (C - 1)] (both empty at degree 0); sh_degree."""
    positions: torch.Tensor
    sh_dc: torch.Tensor
    opacities: torch.Tensor
    scales: torch.Tensor
    rotations: torch.Tensor
    sh_index: torch.Tensor
    sh_codebook: torch.Tensor
    sh_degree: int

    def num_gaussians(self) -> int:
        return int(self.positions.shape[0])


def normalised_rotations(rotations: torch.Tensor) -> torch.Tensor:
    """q / |q| per row, as stored at 16 bits; a zero quaternion stays zero."""
    return rotations / rotations.norm(dim=1, keepdim=True).clamp_min(1e-30)


def compress_gaussians(model: GaussianModel, sh_codes: int = 8192, iters: int = 10,
                       weights: Optional[torch.Tensor] = None, geometry_dtype: torch.dtype = torch.float16,
                       init: Optional[torch.Tensor] = None) -> CompressedGaussians:
    """The SH bands l >= 1 of every Gaussian - the row sh_coeffs[:, :, 1:] as 3 (C - 1) floats - are replaced by the
    index of the nearest of min(sh_codes, N) codes fitted by vq_fit (weights: anything per Gaussian and non-negative,
    ContributionScores.weight_sum for one; init: a first codebook).  Positions stay fp32; the DC colour, opacities,
    scales and rotations are cast to geometry_dtype, the rotations normalised first so that a large raw quaternion
    cannot overflow 16 bits; torch.float32 keeps all of them raw and exact."""
    _torch_check(model.is_valid(), "GaussianModel is not valid")
    _torch_check(model.positions.is_cuda, "GaussianModel must be on CUDA device")
    _torch_check(geometry_dtype in (torch.float16, torch.float32),
                 "compress_gaussians: geometry_dtype must be float16 or float32")
    _torch_check(1 <= int(sh_codes) <= VQ_MAX_CODES, f"compress_gaussians: 1 <= sh_codes <= {VQ_MAX_CODES}")
    n, coeffs = model.num_gaussians(), int(model.sh_coeffs.shape[2])
    _torch_check(coeffs in (1, 4, 9, 16), f"compress_gaussians: sh_coeffs has {coeffs} coefficients, not 1, 4, 9 or 16")
    dev = model.positions.device
    d = 3 * (coeffs - 1)
    sh = model.sh_coeffs.to(torch.float32)
    if d > 0 and n > 0:
        codebook, index, _ = vq_fit(sh[:, :, 1:].reshape(n, d), sh_codes, iters=iters, weights=weights, init=init)
        index = index.to(torch.uint16)
    else:
        codebook = torch.empty((0, d), dtype=torch.float32, device=dev)
        index = torch.empty(n if d > 0 else 0, dtype=torch.uint16, device=dev)
    rot = model.rotations.to(torch.float32)
    if geometry_dtype != torch.float32:
        rot = normalised_rotations(rot)
    g = geometry_dtype
    return CompressedGaussians(positions=model.positions.to(torch.float32).contiguous().clone(),
                               sh_dc=sh[:, :, 0].to(g).contiguous(), opacities=model.opacities.to(g).contiguous(),
                               scales=model.scales.to(g).contiguous(), rotations=rot.to(g).contiguous(),
                               sh_index=index, sh_codebook=codebook, sh_degree=int(math.isqrt(coeffs)) - 1)


def decompress_gaussians(cm: CompressedGaussians, device=None) -> GaussianModel:
    """The GaussianModel a CompressedGaussians stands for: fp32, sh_coeffs [N,3,C] with codebook[index] in the bands."""
    dev = torch.device(device) if device is not None else cm.positions.device
    n, coeffs = cm.num_gaussians(), sh_coeff_count(int(cm.sh_degree))
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    sh = torch.empty((n, 3, coeffs), dtype=torch.float32, device=dev)
    sh[:, :, 0] = f(cm.sh_dc)
    if coeffs > 1:
        rows = f(cm.sh_codebook)[cm.sh_index.to(dev).to(torch.int64)]
        sh[:, :, 1:] = rows.reshape(n, 3, coeffs - 1)
    return GaussianModel(positions=f(cm.positions).clone(), sh_coeffs=sh, opacities=f(cm.opacities).clone(),
                         rotations=f(cm.rotations).clone(), scales=f(cm.scales).clone())


def nbytes(cm: CompressedGaussians) -> int:
    """Payload bytes: the arrays of the container, without the file's directory."""
    return sum(int(getattr(cm, name).numel()) * int(getattr(cm, name).element_size()) for name in _FIELDS)


def _to_numpy(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy()


def write_compressed(path, cm: CompressedGaussians) -> int:
    """An uncompressed .npz of the container's seven arrays and meta = int64 [version, N, sh_degree, K].  Returns the
    file's size."""
    meta = np.array([FORMAT_VERSION, cm.num_gaussians(), int(cm.sh_degree), int(cm.sh_codebook.shape[0])],
                    dtype=np.int64)
    with open(path, "wb") as fh:
        np.savez(fh, meta=meta, **{name: _to_numpy(getattr(cm, name)) for name in _FIELDS})
        return int(fh.tell())


def read_compressed(path, device=None) -> CompressedGaussians:
    """Reads what write_compressed wrote; ValueError for an unknown version, a missing array, or shapes and dtypes
    that do not agree with meta."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    with np.load(path, allow_pickle=False) as z:
        if "meta" not in z.files:
            raise ValueError("read_compressed: no meta array")
        meta = z["meta"]
        if meta.dtype != np.int64 or meta.shape != (4,):
            raise ValueError("read_compressed: meta must be int64 [version, N, sh_degree, K]")
        version, n, degree, k = (int(v) for v in meta)
        if version != FORMAT_VERSION:
            raise ValueError(f"read_compressed: unknown format version {version}")
        if n < 0 or not 0 <= degree <= 3 or not 0 <= k <= VQ_MAX_CODES:
            raise ValueError("read_compressed: meta out of range")
        d = 3 * (sh_coeff_count(degree) - 1)
        shapes = {"positions": (n, 3), "sh_dc": (n, 3), "opacities": (n, 1), "scales": (n, 3), "rotations": (n, 4),
                  "sh_index": (n if d > 0 else 0,), "sh_codebook": (k, d)}
        arrays = {}
        for name in _FIELDS:
            if name not in z.files:
                raise ValueError(f"read_compressed: no array {name}")
            a = z[name]
            if tuple(a.shape) != shapes[name]:
                raise ValueError(f"read_compressed: {name} is {tuple(a.shape)}, meta says {shapes[name]}")
            arrays[name] = a
    geo = {arrays[name].dtype for name in ("sh_dc", "opacities", "scales", "rotations")}
    if (arrays["positions"].dtype != np.float32 or arrays["sh_codebook"].dtype != np.float32 or
            arrays["sh_index"].dtype != np.uint16 or len(geo) != 1 or
            next(iter(geo)) not in (np.dtype(np.float16), np.dtype(np.float32))):
        raise ValueError("read_compressed: array dtypes do not agree with the format")
    if d > 0 and n > 0 and (k == 0 or int(arrays["sh_index"].max()) >= k):
        raise ValueError("read_compressed: an index points past the codebook")

    return CompressedGaussians(**{name: torch.from_numpy(np.ascontiguousarray(arrays[name])).to(dev) for name in _FIELDS},
                               sh_degree=degree)
