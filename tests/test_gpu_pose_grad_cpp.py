"""The camera-pose gradient through the C++ host (adapter/pose_driver.cpp: cugs_hip::render_backward(...,
want_camera_grad = true) with the depth and alpha map gradients) against the Python host on the same inputs."""
import os
import subprocess

import numpy as np
import pytest
import torch

from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "cuda-gaussian-splatting_amd", "adapter", "pose_driver.bin")


def test_cpp_pose_driver_matches_python_host(pkg, dev, tmp_path):
    if not os.path.exists(DRIVER):
        pytest.skip("pose_driver.bin not built (make -C cuda-gaussian-splatting_amd/adapter)")
    w, h, n = 200, 150, 5000
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=3, seed=29, mu_s=-3.8)
    cam = pkg.pose.apply_se3(pkg.scene.make_camera(w, h, view=2), [0.05, -0.03, 0.1, 0.04, -0.06, 0.03])
    rng = np.random.default_rng(4)
    g = pkg.scene.make_dl_dcolor(w, h)
    dD = (rng.standard_normal((h, w)) * 1e-4).astype(np.float32)
    dA = (rng.standard_normal((h, w)) * 1e-4).astype(np.float32)
    files = dict(positions=arrays["positions"], sh=arrays["sh_coeffs"], opacities=arrays["opacities"],
                 rotations=arrays["rotations"], scales=arrays["scales"], dl_dcolor=g, dl_ddepth=dD, dl_dalpha=dA)
    for k, v in files.items():
        np.ascontiguousarray(v, np.float32).tofile(tmp_path / f"{k}.f32")
    abi = cam.to_abi()
    np.array(list(abi.view) + [abi.fx, abi.fy, abi.cx, abi.cy, abi.width, abi.height] + list(abi.cam_center),
             np.float32).tofile(tmp_path / "camera.f32")
    res = subprocess.run([DRIVER, str(tmp_path)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert res.returncode == 0, f"rc={res.returncode} stdout={res.stdout!r} stderr={res.stderr!r}"

    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=3)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    t = lambda a: torch.from_numpy(a).to(dev)
    grads = pkg.render_backward(t(g), out, model, cam, settings, dL_ddepth_map=t(dD), dL_dalpha=t(dA),
                                want_camera_grad=True)
    rd = lambda name: np.fromfile(tmp_path / f"{name}.f32", dtype=np.float32)
    view = rd("d_view").reshape(4, 4)
    want = np_(grads.dL_dviewmat)
    assert (view[3] == 0.0).all() and np.abs(want).max() > 0.0
    # both hosts run the same kernels on the same inputs; the blend backward's scatter (float atomics) may order the
    # accumulator's additions differently from run to run, so the bits agree up to that order
    assert max_err_over_max(view, want) <= 1e-5
    assert max_err_over_max(rd("d_positions"), np_(grads.dL_dpositions).reshape(-1)) <= 1e-5
