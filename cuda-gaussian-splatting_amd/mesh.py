"""Mesh export (not in the reference): fuse render()'s depth and alpha maps into a dense truncated
signed distance volume on the device (cugs_tsdf_integrate, up to 16 views per pass over the volume) and extract the zero
level set as a surface-net mesh (cugs_mesh_plan / cugs_mesh_emit).  The rules, operation by operation, are in
include/cugs_hip.h.  write_mesh_ply assembles the file on the host: not a hot path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._lib import TsdfOpts, TsdfView, TsdfVolume, check, lib
from .rasterizer import _ptr, _stream, _torch_check, render
from .types import CameraInfo, GaussianModel, RenderOutput, RenderSettings

MAX_VIEWS = 16          # CUGS_TSDF_MAX_VIEWS


class Mesh(NamedTuple):
    vertices: torch.Tensor              # [V,3] float32, world
    faces: torch.Tensor                 # [F,3] int32, normals out of the surface (towards free space)
    colors: Optional[torch.Tensor]      # [V,3] float32, or None for a volume without colour


class TSDFView(NamedTuple):
    """One view of TSDFVolume.integrate_views."""
    maps: Union[RenderOutput, Tuple[torch.Tensor, torch.Tensor]]    # a RenderOutput with depth_map, or (depth_map, alpha)
    camera: CameraInfo
    color: Optional[torch.Tensor] = None     # [H,W,3]; default: the RenderOutput's colour
    weight: Optional[torch.Tensor] = None    # [H,W]


class TSDFVolume:
    """A dense box of voxels from bounds = (lo, hi): voxel (0,0,0) is centred on lo, the counts are
    floor((hi - lo) / voxel_size) + 1 per axis, or `dims` = (nx, ny, nz) where given.  planes [P, nz, ny, nx]: tsdf (in
    units of trunc, 1 = free), weight, and with color=True r, g, b."""

    def __init__(self, bounds, voxel_size: float, device, trunc: Optional[float] = None, color: bool = True,
                 max_weight: float = 64.0, min_depth: float = 0.05, dims: Optional[Sequence[int]] = None):
        lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in bounds)
        voxel_size = float(voxel_size)
        _torch_check(0.0 < voxel_size < math.inf, f"voxel_size must be positive and finite, got {voxel_size}")
        _torch_check(bool(np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi >= lo)),
                     f"bounds must be finite with hi >= lo, got {lo}, {hi}")
        trunc = 4.0 * voxel_size if trunc is None else float(trunc)
        _torch_check(0.0 < trunc < math.inf, f"trunc must be positive and finite, got {trunc}")
        _torch_check(0.0 < float(max_weight) < math.inf, f"max_weight must be positive and finite, got {max_weight}")
        _torch_check(0.0 < float(min_depth) < math.inf, f"min_depth must be positive and finite, got {min_depth}")
        dims = [int(math.floor((h - l) / voxel_size + 1e-6)) + 1 for l, h in zip(lo, hi)] if dims is None else [int(d) for d in dims]
        _torch_check(len(dims) == 3 and min(dims) >= 1, f"the voxel counts must be three positive integers, got {dims}")
        _torch_check(dims[0] * dims[1] * dims[2] <= 2 ** 31 - 1, f"{dims} voxels do not fit 2^31 - 1")
        self.device = torch.device(device)
        _torch_check(self.device.type == "cuda", "a TSDFVolume lives on a CUDA device")
        self.nx, self.ny, self.nz = dims
        self.origin = tuple(float(np.float32(v)) for v in lo)
        self.voxel_size, self.trunc = voxel_size, trunc
        self.max_weight, self.min_depth = float(max_weight), float(min_depth)
        self.has_color = bool(color)
        self.planes = torch.zeros((5 if color else 2, self.nz, self.ny, self.nx), dtype=torch.float32, device=self.device)
        self.planes[0].fill_(1.0)

    tsdf = property(lambda self: self.planes[0])
    weight = property(lambda self: self.planes[1])
    color = property(lambda self: self.planes[2:5].permute(1, 2, 3, 0) if self.has_color else None)   # [nz,ny,nx,3] view

    def _abi(self) -> TsdfVolume:
        return TsdfVolume(planes=self.planes.data_ptr(), nx=self.nx, ny=self.ny, nz=self.nz, color=int(self.has_color),
                          origin=(C.c_float * 3)(*self.origin), voxel_size=self.voxel_size, trunc=self.trunc)

    def integrate(self, render_out_or_maps, camera: CameraInfo, color: Optional[torch.Tensor] = None,
                  weight: Optional[torch.Tensor] = None, min_alpha: float = 0.5) -> None:
        """Fuse one view: a RenderOutput of render(..., want_depth_map=True) or the pair (depth_map, alpha)."""
        self.integrate_views([TSDFView(render_out_or_maps, camera, color, weight)], min_alpha=min_alpha)

    def integrate_views(self, views: Sequence[TSDFView], min_alpha: float = 0.5) -> None:
        """Fuse the views in the order given, up to 16 per pass over the volume (the same bits however they are
        batched)."""
        _torch_check(0.0 < float(min_alpha) < math.inf, f"min_alpha must be positive and finite, got {min_alpha}")
        views = [v if isinstance(v, TSDFView) else TSDFView(*v) for v in views]
        vol = self._abi()
        opts = TsdfOpts(min_depth=self.min_depth, min_alpha=float(min_alpha), max_weight=self.max_weight)
        for first in range(0, len(views), MAX_VIEWS):
            batch = views[first:first + MAX_VIEWS]
            table = (TsdfView * len(batch))()
            keep = []                                       # the contiguous copies live until the launch is queued
            for slot, v in zip(table, batch):
                _torch_check(isinstance(v.camera, CameraInfo), f"camera must be a CameraInfo, got {type(v.camera).__name__}")
                h, w = int(v.camera.height), int(v.camera.width)
                if isinstance(v.maps, RenderOutput):
                    _torch_check(v.maps.depth_map is not None,
                                 "the RenderOutput has no depth map (render(..., want_depth_map=True))")
                    depth, alpha = v.maps.depth_map, v.maps.alpha
                    colour = v.maps.color if v.color is None else v.color
                else:
                    depth, alpha = v.maps
                    colour = v.color
                maps = [("depth_map", depth, (h, w)), ("alpha", alpha, (h, w))]
                if self.has_color:
                    _torch_check(colour is not None, "a volume with colour needs a colour image for every view")
                    maps.append(("color", colour, (h, w, 3)))
                if v.weight is not None:
                    maps.append(("weight", v.weight, (h, w)))
                ptrs = {}
                for name, t, shape in maps:
                    _torch_check(tuple(t.shape) == shape, f"{name} must be {shape}, got {tuple(t.shape)}")
                    _torch_check(t.dtype == torch.float32, f"{name} must be float32, got {t.dtype}")
                    _torch_check(t.is_cuda and t.device == self.device, f"{name} must be on the volume's device")
                    t = t.contiguous()
                    keep.append(t)
                    ptrs[name] = t.data_ptr()
                slot.camera = v.camera.to_abi()
                slot.depth_map, slot.alpha = ptrs["depth_map"], ptrs["alpha"]
                slot.color, slot.weight = ptrs.get("color"), ptrs.get("weight")
            check(lib.cugs_tsdf_integrate(C.byref(vol), table, len(batch), C.byref(opts), _stream(self.device)),
                  "cugs_tsdf_integrate")
            for t in keep:                                   # a copy made here may be freed once the stream has used it
                t.record_stream(torch.cuda.current_stream(self.device))

    def extract(self, min_weight: float = 0.0) -> Mesh:
        """The surface-net mesh of the zero level set over the cells whose eight corners all have weight > min_weight.
        Blocks on one small read-back (the counts)."""
        _torch_check(0.0 <= float(min_weight) < math.inf, f"min_weight must be non-negative and finite, got {min_weight}")
        vol = self._abi()
        nbytes = int(lib.cugs_mesh_workspace_bytes(self.nx, self.ny, self.nz))
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        counts = (C.c_int64 * 2)()
        stream = _stream(self.device)
        check(lib.cugs_mesh_plan(C.byref(vol), float(min_weight), _ptr(ws), ws.numel(), counts, stream), "cugs_mesh_plan")
        nv, nf = int(counts[0]), int(counts[1])
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=self.device)
        colors = torch.empty((nv, 3), dtype=torch.float32, device=self.device) if self.has_color else None
        faces = torch.empty((nf, 3), dtype=torch.int32, device=self.device)
        check(lib.cugs_mesh_emit(C.byref(vol), _ptr(ws), ws.numel(), nv, nf, _ptr(vertices), _ptr(colors), _ptr(faces), stream),
              "cugs_mesh_emit")
        ws.record_stream(torch.cuda.current_stream(self.device))
        return Mesh(vertices, faces, colors)


def write_mesh_ply(path: str, mesh: Mesh) -> None:
    """Binary little-endian PLY: float x y z, with colours uchar red green blue (clamped to [0, 1], rounded), then the
    triangles as `list uchar int vertex_indices`."""
    v = mesh.vertices.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
    f = mesh.faces.detach().cpu().numpy().astype("<i4").reshape(-1, 3)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}",
              "property float x", "property float y", "property float z"]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if mesh.colors is not None:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    vert = np.zeros(len(v), dtype=np.dtype(fields))
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if mesh.colors is not None:
        c = mesh.colors.detach().cpu().numpy().reshape(-1, 3).astype(np.float64)
        c = np.floor(np.clip(np.nan_to_num(c), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.zeros(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    face["n"], face["i"] = 3, f
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vert.tobytes())
        out.write(face.tobytes())


def extract_mesh(model: GaussianModel, cameras: Sequence[CameraInfo], settings: RenderSettings, bounds, voxel_size: float,
                 trunc: Optional[float] = None, color: bool = True, max_weight: float = 64.0, min_alpha: float = 0.5,
                 min_weight: float = 0.0, volume: Optional[TSDFVolume] = None) -> Mesh:
    """Render every camera with its depth map, fuse the views in batches of up to 16 and extract the mesh.  `volume`:
    fuse into an existing TSDFVolume (bounds, voxel_size, trunc, color and max_weight are then its own)."""
    if volume is None:
        volume = TSDFVolume(bounds, voxel_size, model.positions.device, trunc=trunc, color=color, max_weight=max_weight)
    batch = []
    for cam in cameras:
        batch.append(TSDFView(render(model, cam, settings, for_backward=False, want_depth_map=True), cam))
        if len(batch) == MAX_VIEWS:
            volume.integrate_views(batch, min_alpha=min_alpha)
            batch = []
    if batch:
        volume.integrate_views(batch, min_alpha=min_alpha)
    return volume.extract(min_weight=min_weight)
