"""Host-side mirror of the reference's point-cloud initialisation (core/gaussian_init.{hpp,cpp}) over csrc/knn.hip.

init_gaussians_from_sparse(positions, colors, sh_degree, k_neighbors) is the reference's function of that name
(gaussian_init.cpp:72-152, the first thing Trainer::Trainer calls, trainer.cpp:61) with the SparsePoint span taken
apart into positions [n, 3] float32 and colors [n, 3] uint8; the model comes back on the device, rows in the input
order of the points.  knn_mean_distances is its compute_knn_mean_distances (:25-68): exact, on the device, by an
exhaustive or a tree search that give the same bits.

Differences from the reference, all at the boundary:
  * the k square roots are added in ascending order (the reference adds them in whatever order nth_element left
    them): at most k ulp of the mean apart;
  * the model lives on the device (the reference builds CPU tensors and moves them later);
  * no log line (spdlog), hence no min / max read-back of the scales.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ._lib import KNN_AUTO, KNN_EXHAUSTIVE, KNN_TREE, check, lib
from .rasterizer import _ptr, _skey, _stream, _torch_check
from .types import GaussianModel, K_MAX_SH_DEGREE, sh_coeff_count

ROUTES = {"auto": KNN_AUTO, "exhaustive": KNN_EXHAUSTIVE, "tree": KNN_TREE}
K_MAX_NEIGHBORS = 16

_workspaces: Dict[tuple, torch.Tensor] = {}


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """Grow-only scratch per (device, stream), as the other stages keep it."""
    key = _skey(device)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def _device(device, *tensors) -> torch.device:
    if device is not None:
        dev = torch.device(device)
    else:
        dev = next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cuda"))
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _to_device(a, dtype: torch.dtype, dev: torch.device) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


def _positions(positions, dev: torch.device) -> torch.Tensor:
    _torch_check(len(positions.shape) == 2 and positions.shape[1] == 3, "positions must be [N, 3]")
    return _to_device(positions, torch.float32, dev)


def _mean_distances(pos: torch.Tensor, k_neighbors: int, route: str) -> torch.Tensor:
    _torch_check(route in ROUTES, f"route must be one of {sorted(ROUTES)}, got {route!r}")
    _torch_check(1 <= int(k_neighbors) <= K_MAX_NEIGHBORS,
                 f"k_neighbors must be 1..{K_MAX_NEIGHBORS}, got {k_neighbors}")
    n, dev = int(pos.shape[0]), pos.device
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        ws = None
        if ROUTES[route] != KNN_EXHAUSTIVE:
            ws = _workspace(dev, lib.cugs_knn_workspace_bytes(n, int(k_neighbors)))
        check(lib.cugs_knn_mean_distances(n, int(k_neighbors), _ptr(pos), _ptr(out), _ptr(ws),
                                          ws.numel() if ws is not None else 0, ROUTES[route], _stream(dev)),
              "cugs_knn_mean_distances")
    return out


def knn_mean_distances(positions, k_neighbors: int = 3, route: str = "auto", device=None) -> torch.Tensor:
    """Mean distance from every point to its k nearest other points (gaussian_init.cpp:25-68): float32 [n] on the
    device, in the input order.  k is clamped to n - 1; n == 1 gives 1."""
    return _mean_distances(_positions(positions, _device(device, positions)), k_neighbors, route)


def init_gaussians_from_sparse(positions, colors, sh_degree: int = 3, k_neighbors: int = 3, device=None,
                               route: str = "auto") -> GaussianModel:
    """gaussian_init.cpp:72-152.  positions [n, 3] float32, colors [n, 3] uint8 (numpy arrays or tensors)."""
    _torch_check(0 <= int(sh_degree) <= K_MAX_SH_DEGREE,
                 f"SH degree must be 0..{K_MAX_SH_DEGREE}, got {sh_degree}")                   # :77-78
    dev = _device(device, positions, colors)
    pos = _positions(positions, dev)
    n = int(pos.shape[0])
    _torch_check(tuple(colors.shape) == (n, 3), "colors must be [N, 3]")
    _torch_check((colors.dtype == torch.uint8) if isinstance(colors, torch.Tensor) else (colors.dtype == np.uint8),
                 "colors must be uint8")
    col = _to_device(colors, torch.uint8, dev)
    C = sh_coeff_count(int(sh_degree))
    f = dict(dtype=torch.float32, device=dev)
    model = GaussianModel(positions=torch.empty((n, 3), **f), sh_coeffs=torch.empty((n, 3, C), **f),
                          opacities=torch.empty((n, 1), **f), rotations=torch.empty((n, 4), **f),
                          scales=torch.empty((n, 3), **f))
    if n == 0:                                                                                   # :88-95
        return model
    m = _mean_distances(pos, k_neighbors, route)
    with torch.cuda.device(dev):
        check(lib.cugs_init_from_points(n, C, _ptr(pos), _ptr(col), _ptr(m), _ptr(model.positions),
                                        _ptr(model.sh_coeffs), _ptr(model.opacities), _ptr(model.rotations),
                                        _ptr(model.scales), _stream(dev)), "cugs_init_from_points")
    return model
