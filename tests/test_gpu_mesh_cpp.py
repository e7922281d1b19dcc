"""Mesh export through the C++ host (cuda-gaussian-splatting_amd/adapter: cugs_hip::tsdf_integrate and mesh_extract) run
as a native program (adapter/mesh_driver.bin) on the fused sphere of tests/tsdf_cases.py: the bytes of the Python host in
the planes, the vertices, the colours and the faces."""
import os
import sys

import numpy as np
import pytest
import torch            # before the package, as in every GPU test module: its library binds to the HIP runtime torch loads

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as cases      # noqa: E402
import tsdf_ref as R            # noqa: E402
from cpp_driver import run_driver

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("box,color", [("odd", True), ("aligned", False)])
def test_cpp_mesh_matches_python_host(pkg, dev, tmp_path, box, color):
    dims, origin = cases.BOXES[box]
    views = cases.sphere_views(color)
    flt = lambda x: repr(float(np.float32(x)))               # the float32 values, written so that they read back exactly
    manifest = [f"volume {dims[0]} {dims[1]} {dims[2]} {int(color)} " + " ".join(flt(x) for x in (*origin, cases.VS, cases.TRUNC,
                                                                                                  R.MAX_WEIGHT, R.MIN_DEPTH)),
                f"views {len(views)} {flt(R.MIN_ALPHA)} {flt(0.0)}"]
    for i, v in enumerate(views):
        manifest.append(f"{v['H']} {v['W']} " + " ".join(flt(v[k]) for k in ("fx", "fy", "cx", "cy")) + f" {int(v['weight'] is not None)}")
        np.concatenate([v["m"].reshape(-1), np.array([0, 0, 0, 1], np.float32)]).astype(np.float32).tofile(tmp_path / f"view_{i}_m.f32")
        v["D"].tofile(tmp_path / f"view_{i}_d.f32")
        v["A"].tofile(tmp_path / f"view_{i}_a.f32")
        if color:
            v["color"].tofile(tmp_path / f"view_{i}_c.f32")
        if v["weight"] is not None:
            v["weight"].tofile(tmp_path / f"view_{i}_w.f32")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")

    res = run_driver("mesh_driver", tmp_path)

    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam = lambda v: pkg.CameraInfo(width=v["W"], height=v["H"],
                                   intrinsics=pkg.CameraIntrinsics(fx=float(v["fx"]), fy=float(v["fy"]), cx=float(v["cx"]),
                                                                   cy=float(v["cy"])),
                                   rotation=v["m"][:, :3].copy(), translation=v["m"][:, 3].copy())
    vol = pkg.TSDFVolume((origin, origin), cases.VS, dev, trunc=cases.TRUNC, color=color, dims=dims)
    vol.integrate_views([pkg.TSDFView((up(v["D"]), up(v["A"])), cam(v), up(v["color"]), up(v["weight"])) for v in views])
    mesh = vol.extract()
    assert f"mesh_driver ok views={len(views)} vertices={len(mesh.vertices)} faces={len(mesh.faces)} bad_args_throw={int(color)}" \
        in res.stdout, res.stdout
    assert len(mesh.vertices) > 1000 and len(mesh.faces) > 1500
    got = lambda name, dt: np.fromfile(tmp_path / name, dt)
    assert got("out_planes.f32", np.float32).tobytes() == vol.planes.cpu().numpy().tobytes()
    assert got("out_vertices.f32", np.float32).tobytes() == mesh.vertices.cpu().numpy().tobytes()
    assert got("out_faces.i32", np.int32).tobytes() == mesh.faces.cpu().numpy().tobytes()
    if color:
        assert got("out_colors.f32", np.float32).tobytes() == mesh.colors.cpu().numpy().tobytes()
