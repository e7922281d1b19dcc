"""Mesh export on the device against its numpy mirror tests/tsdf_ref.py, byte for byte:
cugs_tsdf_integrate (planes and the set of touched voxels), cugs_mesh_plan / cugs_mesh_emit (vertices, colours, faces),
and the Python layer (TSDFVolume, extract_mesh, write_mesh_ply).  The scenes are those of tests/tsdf_cases.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch            # before the package, as in every GPU test module: its library binds to the HIP runtime torch loads

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as cases      # noqa: E402
import tsdf_ref as R            # noqa: E402

f32 = np.float32


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    if a.tobytes() != b.tobytes():
        diff = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))
        raise AssertionError(f"{what}: {len(diff)} bytes differ, the first at byte {diff[0]}")


def _camera(pkg, view):
    return pkg.CameraInfo(width=view["W"], height=view["H"],
                          intrinsics=pkg.CameraIntrinsics(fx=float(view["fx"]), fy=float(view["fy"]), cx=float(view["cx"]),
                                                          cy=float(view["cy"])),
                          rotation=view["m"][:, :3].copy(), translation=view["m"][:, 3].copy())


def _to_gpu(pkg, dev, views):
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return [pkg.TSDFView((up(v["D"]), up(v["A"])), _camera(pkg, v), up(v["color"]), up(v["weight"])) for v in views]


def _volume(pkg, dev, dims, origin, color, max_weight=R.MAX_WEIGHT, planes=None, misalign=False):
    vol = pkg.TSDFVolume((origin, origin), cases.VS, dev, trunc=cases.TRUNC, color=color, max_weight=max_weight,
                         min_depth=R.MIN_DEPTH, dims=dims)
    if misalign:                                             # the same planes, one float off a 16-byte boundary
        buf = torch.empty(vol.planes.numel() + 1, dtype=torch.float32, device=dev)
        view = buf[1:].view(vol.planes.shape)
        view.copy_(vol.planes)
        vol.planes = view
        assert vol.planes.data_ptr() % 16 == 4
    if planes is not None:
        vol.planes.copy_(torch.from_numpy(planes).to(dev))
    return vol


@functools.lru_cache(maxsize=None)
def _mirror_fused(box, color):
    """(planes, touched, samples) of the eight views in the mirror; computed once, never modified."""
    dims, origin = cases.BOXES[box]
    planes = R.new_planes(dims, color)
    samples = []
    touched = R.integrate(planes, origin, cases.VS, cases.TRUNC, cases.sphere_views(color), samples=samples)
    planes.setflags(write=False)
    return planes, touched, samples


def test_camera_list_covers_the_cases():
    """Each case the camera list is there for really occurs in the mirror (no GPU needed)."""
    _, touched, samples = _mirror_fused("odd", True)
    views = cases.sphere_views(True)
    assert touched.any() and not touched.all()
    inside_box = samples[6]
    assert (inside_box["zc"] < 0).any()                                               # voxels behind the camera
    assert ((inside_box["zc"] > 0) & (inside_box["zc"] <= f32(R.MIN_DEPTH))).any()   # in front, within min_depth
    s = samples[7]
    W, H = cases.W, cases.H
    fr = s["front"]
    assert (fr & (s["u"] > -1) & (s["u"] < 0)).any() and (fr & (s["u"] >= W) & (s["u"] < W + 1)).any()
    assert (fr & (s["v"] > -1) & (s["v"] < 0)).any() and (fr & (s["v"] >= H) & (s["v"] < H + 1)).any()
    assert not (s["inside"] & ((s["u"] < 0) | (s["u"] >= W) | (s["v"] < 0) | (s["v"] >= H))).any()
    assert any(v["weight"] is None for v in views) and any(v["weight"] is not None for v in views)
    assert all(v["color"] is not None for v in views) and all(v["color"] is None for v in cases.sphere_views(False))
    for smp in samples:                                                               # every view touches something
        assert smp["ok"].any()
    assert _mirror_fused("single", True)[1].all()                                     # the single voxel is touched


@pytest.mark.gpu
@pytest.mark.parametrize("box,color", [("odd", True), ("odd", False), ("aligned", True), ("aligned", False),
                                       ("single", True), ("single", False)])
def test_integrate_matches_mirror(pkg, dev, box, color):
    dims, origin = cases.BOXES[box]
    planes, touched, _ = _mirror_fused(box, color)
    vol = _volume(pkg, dev, dims, origin, color)
    assert (vol.planes.data_ptr() % 16 == 0)
    vol.integrate_views(_to_gpu(pkg, dev, cases.sphere_views(color)))
    got = vol.planes.cpu().numpy()
    _same(got, planes, f"planes of the {box} box")
    assert np.array_equal(got[1] > 0, touched)               # the set of touched voxels: the weight starts at 0
    assert vol.tsdf.shape == (dims[2], dims[1], dims[0]) and vol.weight.shape == vol.tsdf.shape
    assert (vol.color.shape == vol.tsdf.shape + (3,)) if color else vol.color is None


@pytest.mark.gpu
def test_integrate_special_pixels_and_weight_cap(pkg, dev):
    """Alpha at and below min_alpha, depth 0 and NaN, weight 0 and NaN; then max_weight = 3 with the view five times."""
    dims, origin = cases.BOXES["odd"]
    view = cases.edge_case_view(True)
    s = R.sample(dims, origin, cases.VS, cases.TRUNC, view)
    hit = lambda lo, hi, mask: (mask & (s["iu"] >= lo) & (s["iu"] < hi)).any()
    assert hit(30, 36, s["inside"] & (s["A"] == f32(0.5))) and not hit(30, 36, s["seen"])      # alpha at min_alpha
    assert hit(36, 42, s["inside"] & (s["A"] > 0) & (s["A"] < f32(0.5)))                        # below it
    assert hit(42, 48, s["seen"]) and not hit(42, 48, s["ok"] & (s["zc"] > f32(cases.TRUNC)))  # depth 0
    assert hit(48, 54, s["seen"] & np.isnan(s["sdf"])) and not hit(48, 54, s["ok"])            # depth NaN
    assert hit(54, 60, s["seen"] & (s["w"] == 0)) and not hit(54, 60, s["weighted"])           # weight 0
    assert hit(60, 66, s["seen"] & np.isnan(s["w"])) and not hit(60, 66, s["weighted"])        # weight NaN
    assert hit(66, 72, s["ok"]) and hit(0, 30, s["ok"] & (s["A"] == f32(0.8)))
    ref = R.new_planes(dims, True)
    R.integrate(ref, origin, cases.VS, cases.TRUNC, [view] * 5, max_weight=3.0)
    assert (ref[1] == 3.0).any() and ref[1].max() == 3.0                               # the cap binds
    gpu_view = _to_gpu(pkg, dev, [view])
    once = _volume(pkg, dev, dims, origin, True, max_weight=3.0)
    once.integrate_views(gpu_view * 5)
    _same(once.planes.cpu().numpy(), ref, "one call of five")
    five = _volume(pkg, dev, dims, origin, True, max_weight=3.0)
    for _ in range(5):
        five.integrate(*gpu_view[0], min_alpha=R.MIN_ALPHA)
    _same(five.planes.cpu().numpy(), ref, "five calls of one")
    assert not np.isnan(ref).any()


@pytest.mark.gpu
@pytest.mark.parametrize("box", ["odd", "aligned"])
def test_integrate_batching_leaves_the_same_bytes(pkg, dev, box):
    """Sixteen views in one call, sixteen single calls, 8 + 8, and 4 + 12 onto an earlier call's result."""
    dims, origin = cases.BOXES[box]
    views = cases.sphere_views(True) * 2
    ref = R.new_planes(dims, True)
    R.integrate(ref, origin, cases.VS, cases.TRUNC, views)
    gpu_views = _to_gpu(pkg, dev, views)
    for split in ((16,), (1,) * 16, (8, 8), (4, 12)):
        vol = _volume(pkg, dev, dims, origin, True)
        first = 0
        for n in split:
            vol.integrate_views(gpu_views[first:first + n])
            first += n
        _same(vol.planes.cpu().numpy(), ref, f"{box} box, calls of {split}")
    # a second call accumulates on the first: the eight views once are not the eight views twice
    assert not np.array_equal(ref, _mirror_fused(box, True)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("color", [True, False])
def test_integrate_unaligned_base(pkg, dev, color):
    """A volume whose base is one float off a 16-byte boundary takes the 4-byte route: the bytes of the aligned one."""
    dims, origin = cases.BOXES["aligned"]
    vol = _volume(pkg, dev, dims, origin, color, misalign=True)
    vol.integrate_views(_to_gpu(pkg, dev, cases.sphere_views(color)))
    _same(vol.planes.cpu().numpy(), _mirror_fused("aligned", color)[0], "unaligned base")


@functools.lru_cache(maxsize=None)
def _extraction_cases():
    return cases.extraction_volumes()


def _check_extract(pkg, dev, planes, origin, vs, min_weight, what):
    P, nz, ny, nx = planes.shape
    V, C, F = R.surface_nets(planes, origin, vs, min_weight)
    vol = pkg.TSDFVolume((origin, origin), vs, dev, trunc=cases.TRUNC, color=P == 5, dims=(nx, ny, nz))
    vol.planes.copy_(torch.from_numpy(planes).to(dev))
    mesh = vol.extract(min_weight=min_weight)
    assert mesh.vertices.shape == (len(V), 3) and mesh.faces.shape == (len(F), 3), \
        f"{what}: {tuple(mesh.vertices.shape)}, {tuple(mesh.faces.shape)} against {len(V)}, {len(F)}"
    _same(mesh.vertices.cpu().numpy(), V, f"{what}: vertices")
    _same(mesh.faces.cpu().numpy(), F, f"{what}: faces")
    if P == 5:
        _same(mesh.colors.cpu().numpy(), C, f"{what}: colours")
    else:
        assert mesh.colors is None
    again = vol.extract(min_weight=min_weight)               # the same bytes from run to run
    _same(again.vertices.cpu().numpy(), V, f"{what}: vertices again")
    _same(again.faces.cpu().numpy(), F, f"{what}: faces again")
    return V, C, F


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["analytic", "fused", "fused_min_weight", "cut_by_box", "invalid_corners", "ambiguous",
                                  "all_positive", "thin", "analytic_colour"])
def test_extract_matches_mirror(pkg, dev, name):
    planes, origin, min_weight = _extraction_cases()[name]
    V, C, F = _check_extract(pkg, dev, planes, origin, cases.VS, min_weight, name)
    st = R.mesh_stats(V, F) if len(F) else None
    if name in ("all_positive", "thin"):
        assert len(V) == 0 and len(F) == 0                   # {0, 0}, and nothing faults
    elif name == "analytic":
        assert st["edge_counts"] == [0, 0, st["E"]] and st["euler"] == 2 and st["volume"] > 0
    elif name in ("fused", "cut_by_box", "invalid_corners", "fused_min_weight"):
        assert st["edge_counts"][1] > 0                      # open: holes, or the surface leaves the box
        assert len(V) != 1300                                # not the analytic sphere's mesh
    elif name == "ambiguous":
        # both ambiguous cells (corners 0 and 7 against the rest) are active and carry a vertex
        neg = planes[0] < 0
        cells = [(2, 2, 2), (2, 2, 5)]
        for z, y, x in cells:
            c = neg[z:z + 2, y:y + 2, x:x + 2].reshape(-1)
            assert c[0] == c[7] and (c[1:7] != c[0]).all()
        assert st["directed_max"] == 1


@pytest.mark.gpu
def test_extract_scan_levels(pkg, dev):
    """71 x 63 x 59 = 263,907 cells: 258 chunks of 1024 cells (the first scan level: more than one chunk) in two blocks of
    256 chunks (the second level: past 262,144 cells), so the third level adds a non-zero prefix to the second block.
    The third level's own stride of 256 blocks begins at 67 million cells: not reached by a test of seconds."""
    planes, origin = cases.scan_volume()
    assert planes.shape[1:] == (60, 64, 72)
    V, C, F = _check_extract(pkg, dev, planes, origin, 0.1, 0.0, "scan levels")
    # vertices on both sides of cell 262,144 and of a chunk boundary
    cell = np.floor((V.astype(np.float64) - np.array(origin)) / 0.1 - 1e-3).astype(np.int64)
    index = (cell[:, 2] * 63 + cell[:, 1]) * 71 + cell[:, 0]
    assert (index < 262144).any() and (index >= 262144).any()
    assert len(np.unique(index // 1024)) > 100
    assert F.max() == len(V) - 1 and (F >= (index < 262144).sum()).any()


@functools.lru_cache(maxsize=None)
def _small_scene():
    return dict(n=4000, w=128, h=96, lo=(-1.55, -1.55, 1.05), voxel=0.1, dims=(32, 32, 32), min_alpha=0.5)


@pytest.mark.gpu
def test_extract_mesh_on_a_small_model(pkg, dev):
    """extract_mesh = render each camera, fuse, extract: equal to the mirror fed with the GPU's own rendered maps (this
    compares the fusion and the extraction, not the renderer)."""
    sc = _small_scene()
    arrays = pkg.scene.make_gaussians(sc["n"], sc["w"], sc["h"])
    arrays["scales"] = arrays["scales"] + f32(2.3)            # splats large enough to cover pixels: alpha > min_alpha
    arrays["opacities"] = arrays["opacities"] + f32(2.0)
    model = pkg.scene.to_model(arrays, dev)
    cams = [pkg.scene.make_camera(sc["w"], sc["h"], view=k) for k in range(4)]
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=3)
    hi = tuple(l + sc["voxel"] * (d - 1) for l, d in zip(sc["lo"], sc["dims"]))
    mesh = pkg.extract_mesh(model, cams, settings, (sc["lo"], hi), sc["voxel"], min_alpha=sc["min_alpha"])
    planes = R.new_planes(sc["dims"], True)
    views = []
    for cam in cams:
        out = pkg.render(model, cam, settings, for_backward=False, want_depth_map=True)
        K = cam.intrinsics
        views.append(R.make_view(cam.rotation, cam.translation, K.fx, K.fy, K.cx, K.cy, cam.width, cam.height,
                                 out.depth_map.cpu().numpy(), out.alpha.cpu().numpy(), out.color.cpu().numpy()))
    touched = R.integrate(planes, sc["lo"], sc["voxel"], 4 * sc["voxel"], views, min_alpha=sc["min_alpha"])
    V, C, F = R.surface_nets(planes, sc["lo"], sc["voxel"])
    print(f"small model: {int(touched.sum())} of {touched.size} voxels touched, {len(V)} vertices, {len(F)} faces")
    assert touched.sum() > 1000 and len(V) > 50 and len(F) > 20
    _same(mesh.vertices.cpu().numpy(), V, "extract_mesh: vertices")
    _same(mesh.colors.cpu().numpy(), C, "extract_mesh: colours")
    _same(mesh.faces.cpu().numpy(), F, "extract_mesh: faces")
    # the same through a TSDFVolume by hand, one view at a time
    vol = pkg.TSDFVolume((sc["lo"], hi), sc["voxel"], dev)
    assert (vol.nx, vol.ny, vol.nz) == sc["dims"] and vol.trunc == 4 * sc["voxel"]
    for cam in cams:
        vol.integrate(pkg.render(model, cam, settings, for_backward=False, want_depth_map=True), cam, min_alpha=sc["min_alpha"])
    _same(vol.planes.cpu().numpy(), planes, "TSDFVolume.integrate: planes")


def _read_ply(path):
    """A minimal reader of the binary little-endian PLY that write_mesh_ply writes."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[2])
    props = [l.split()[1:] for l in lines if l.startswith("property") and "list" not in l]
    assert "property list uchar int vertex_indices" in lines
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    vert = np.frombuffer(data, dt, nv, end)
    face = np.frombuffer(data, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), nf, end + nv * dt.itemsize)
    assert end + nv * dt.itemsize + nf * 13 == len(data)
    return vert, face


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["analytic", "analytic_colour", "all_positive"])
def test_write_mesh_ply_reads_back(pkg, dev, name, tmp_path):
    planes, origin, min_weight = _extraction_cases()[name]
    P, nz, ny, nx = planes.shape
    vol = pkg.TSDFVolume((origin, origin), cases.VS, dev, trunc=cases.TRUNC, color=P == 5, dims=(nx, ny, nz))
    vol.planes.copy_(torch.from_numpy(planes).to(dev))
    mesh = vol.extract(min_weight)
    path = str(tmp_path / "mesh.ply")
    pkg.write_mesh_ply(path, mesh)
    vert, face = _read_ply(path)
    V = mesh.vertices.cpu().numpy()
    assert len(vert) == len(V) and len(face) == len(mesh.faces)
    _same(np.stack([vert["x"], vert["y"], vert["z"]], 1), V, "ply vertices")
    assert (face["n"] == 3).all()
    _same(np.ascontiguousarray(face["i"]), mesh.faces.cpu().numpy(), "ply faces")
    if P == 5:
        c = mesh.colors.cpu().numpy().astype(np.float64)
        want = np.floor(np.clip(c, 0, 1) * 255 + 0.5).astype(np.uint8)
        _same(np.stack([vert["red"], vert["green"], vert["blue"]], 1), want, "ply colours")
    else:
        assert vert.dtype.names == ("x", "y", "z")
