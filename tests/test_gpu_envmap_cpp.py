"""The environment-map composite and its backward through the C++ host (cuda-gaussian-splatting_amd/adapter:
cugs_hip::EnvironmentMap, composite_environment / _backward, composite_background / _backward) run as a native program
(adapter/envmap_driver.bin) on the same raw inputs as the Python host: the same bytes in every output."""

import numpy as np
import pytest
import torch

import envmap_ref as er
from cpp_driver import run_driver, write_camera, write_f32
from util import np_

pytestmark = pytest.mark.gpu


def test_cpp_envmap_matches_python_host(pkg, dev, tmp_path):
    h, w = er.SHAPES[0]
    res, bound = 16, 1.0
    cam = er.cameras(h, w)["oblique"]
    orient = er.orientation_tilted()
    E, C, T, g = er.case_data(h, w, res)
    info = pkg.CameraInfo(width=w, height=h, rotation=np.array(cam["R"], np.float32),
                          intrinsics=pkg.CameraIntrinsics(cam["fx"], cam["fy"], cam["cx"], cam["cy"]))
    write_camera(tmp_path / "camera.f32", info)
    np.ascontiguousarray(orient, np.float64).tofile(tmp_path / "orientation.f64")
    write_f32(tmp_path, env=E, color=C, final_T=T, g=g)
    (tmp_path / "manifest.txt").write_text(f"{res} {bound}\n")

    res_ = run_driver("envmap_driver", tmp_path)
    assert f"envmap_driver ok res={res} throws=3" in res_.stdout

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    env = pkg.EnvironmentMap(resolution=res, device=dev, orientation=orient)
    env.texture.copy_(t(E))
    out = pkg.RenderOutput(t(C), t(T), *[None] * 9)
    out.depths = torch.zeros(1, device=dev)
    sample = env.sample(info)
    back = pkg.composite_environment_backward(t(g), out, info, env, grad_bound=bound)
    bg_alpha, bg_grad = pkg.composite_background_backward(t(g), out.final_T, sample)
    want = {"image": pkg.composite_environment(out, info, env), "sample": sample, "dalpha": back.dL_dalpha,
            "denv": back.dL_denv, "bg_image": pkg.composite_background(out.color, out.final_T, sample),
            "bg_dalpha": bg_alpha, "bg_dbg": bg_grad}
    for k, v in want.items():
        got = np.fromfile(tmp_path / f"out_{k}.f32", np.float32)
        assert got.tobytes() == np_(v).tobytes(), k
    assert np.fromfile(tmp_path / "out_clamped.i32", np.int32).tolist() == [int(back.clamped)] == [0]
