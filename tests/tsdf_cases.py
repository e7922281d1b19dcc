"""The fixed scenes of tests/test_gpu_tsdf.py and tests/test_gpu_mesh_cpp.py: boxes, the camera list, the maps and the
volumes for extraction.  Everything here is numpy on the host (tests/tsdf_ref.py); nothing touches the GPU."""
import numpy as np

import tsdf_ref as R

f32 = np.float32
CENTRE, RADIUS = (0.03, -0.02, 0.01), 0.83
W, H, FX, FY, CX, CY = 96, 72, 90.0, 90.0, 48.3, 35.6
VS, TRUNC = 0.1, 0.4
ORIGIN = (-1.8, -1.4, -1.1)
# name -> (dims, origin): the odd box (4-byte route), the aligned one (16-byte route), a single voxel just outside the
# sphere on the +z side
BOXES = {
    "odd": ((37, 29, 23), ORIGIN),
    "aligned": ((40, 32, 24), ORIGIN),
    "single": ((1, 1, 1), (0.03, -0.02, 0.94)),
}
# (eye, target).  0-5 along the axes; 6 sits inside the box, so voxels fall behind it and within min_depth of it; 7 is
# close and aimed off-centre, so the box straddles the image edges and voxel centres project to u, v in (-1, 0) and
# [W, W + 1), [H, H + 1).  Odd views carry a weight map.
CAMERAS = [
    ((3.0, 0.2, 0.3), (0, 0, 0)), ((-3.0, 0.4, -0.2), (0, 0, 0)), ((0.3, 3.0, 0.2), (0, 0, 0)), ((0.2, -3.0, 0.4), (0, 0, 0)),
    ((0.1, 0.3, 3.0), (0, 0, 0)), ((0.2, -0.2, -3.0), (0, 0, 0)), ((1.2, 0.9, 0.7), (0, 0, 0)), ((0.5, 0.3, 2.5), (0.9, 0.6, 0.0)),
]


def sphere_views(color=True, cameras=CAMERAS):
    rng = np.random.default_rng(20240611)
    views = []
    for i, (eye, target) in enumerate(cameras):
        Rm, t = R.look_at(eye, target)
        D, A = R.sphere_maps(Rm, t, FX, FY, CX, CY, W, H, CENTRE, RADIUS)
        col = rng.random((H, W, 3), dtype=f32)
        wgt = (0.5 + 1.5 * rng.random((H, W), dtype=f32)).astype(f32)
        views.append(R.make_view(Rm, t, FX, FY, CX, CY, W, H, D, A, col if color else None, wgt if i % 2 else None))
    return views


def edge_case_view(color=True):
    """View 0 with stripes of special pixels: alpha 0.8 (a real division) on the top half, then columns of alpha at
    min_alpha, alpha below it, depth 0, depth NaN, weight 0, weight NaN."""
    v = sphere_views(color)[0]
    D, A = v["D"].copy(), v["A"].copy()
    wgt = np.ones((H, W), f32)
    A[:H // 2] *= f32(0.8)
    D[:H // 2] *= f32(0.8)
    A[:, 30:36] = np.where(A[:, 30:36] > 0, f32(0.5), A[:, 30:36])         # at min_alpha: skipped
    A[:, 36:42] *= f32(0.3)
    D[:, 36:42] *= f32(0.3)                                                   # below min_alpha
    D[:, 42:48] = 0.0
    D[:, 48:54] = np.nan
    wgt[:, 54:60] = 0.0
    wgt[:, 60:66] = np.nan
    wgt[:, 66:72] = f32(2.5)
    return dict(v, D=D, A=A, weight=wgt)


def fused_sphere(box="odd", color=True):
    """(planes, origin, views): the eight views fused by the mirror."""
    dims, origin = BOXES[box]
    planes = R.new_planes(dims, color)
    views = sphere_views(color)
    R.integrate(planes, origin, VS, TRUNC, views)
    return planes, origin, views


def extraction_volumes():
    """name -> (planes, origin, min_weight)."""
    dims, origin = BOXES["odd"]
    out = {}
    out["analytic"] = (R.sphere_volume(dims, origin, VS, TRUNC, CENTRE, RADIUS), origin, 0.0)
    out["fused"] = (fused_sphere("odd", True)[0], origin, 0.0)
    out["fused_min_weight"] = (fused_sphere("odd", True)[0], origin, 1.5)
    out["cut_by_box"] = (R.sphere_volume(dims, origin, VS, TRUNC, CENTRE, 1.35), origin, 0.0)
    holes = R.sphere_volume(dims, origin, VS, TRUNC, CENTRE, RADIUS)
    rng = np.random.default_rng(7)
    near = np.argwhere(np.abs(holes[0]) < 0.5)
    for z, y, x in near[rng.choice(len(near), 12, replace=False)]:
        holes[1, z, y, x] = 0.0                                               # a few corners near the surface invalid
    out["invalid_corners"] = (holes, origin, 0.0)
    # the two diagonal-corner ambiguous cells: corners 0 and 7 inside, and its complement, in a field of +1
    amb = np.ones((2, 6, 6, 9), f32)
    amb[0, 2, 2, 2] = amb[0, 3, 3, 3] = -0.5
    amb[0, 2:4, 2:4, 5:7] = -0.25
    amb[0, 2, 2, 5] = amb[0, 3, 3, 6] = 0.75
    out["ambiguous"] = (amb, (0.0, 0.0, 0.0), 0.0)
    out["all_positive"] = (np.ones((2, 7, 6, 5), f32), (0.0, 0.0, 0.0), 0.0)
    out["thin"] = (R.sphere_volume((9, 1, 8), (-0.4, 0.0, -0.4), VS, TRUNC, (0, 0, 0), 0.25), (-0.4, 0.0, -0.4), 0.0)
    col = R.sphere_volume((12, 11, 10), (-0.55, -0.5, -0.45), VS, TRUNC, (0.01, 0.02, 0.0), 0.33)
    col = np.concatenate([col, np.random.default_rng(3).random((3, 10, 11, 12), dtype=f32)])
    out["analytic_colour"] = (col, (-0.55, -0.5, -0.45), 0.0)
    return out


def scan_volume(dims=(72, 64, 60)):
    """A sphere in a box of 71 x 63 x 59 = 263,907 cells: more than one 1024-cell chunk and, past 262,144 cells, more
    than one 256-chunk block of the second scan level; the sphere reaches the top slab of cells, so both blocks hold
    vertices; only the surface band is non-trivial."""
    origin = tuple(-0.05 * (d - 1) for d in dims)
    return R.sphere_volume(dims, origin, 0.1, 0.4, (0.02, -0.03, 0.3), 2.7), origin
